// The one statement of the pass workspace's sizes and of the time-split tables' layout (csrc/plan.h: pass_bytes,
// SegLayout), printed for a list of geometries so that tests/test_workspace_host_check.py can hold every number to the
// expressions the executor and the stream used to spell out on their own.  Stand-alone: plan.h and nothing else.
//
//   workspace_host_check  F,S,cmap_rows,clips,lag,yin,obs,n_mels,pyin,mel,debug,prop,tsplit,nk,n_seg,tube_cap,tube_rec,seg64,seg32,n_lock ...
//
// One JSON object per argument, in a list.
//
//   workspace_host_check launch_rule
//
// Which Viterbi launch follows chunk k's observations (PassPlan::viterbi_behind) and how many chunks the sequential kernel
// runs (PassPlan::sequential_chunks), for hand-written plans of every pass kind, against the answers written out below:
// one JSON object per plan, exit status 1 when an answer differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../spectrogram-midi_amd/csrc/plan.h"

using namespace aegis;

struct RuleCase {
    const char *name;
    bool persistent, tsplit, hybrid;
    std::vector<int64_t> cb;
    int64_t hyb_S;
    const char *behind;      // per chunk: n(one), s(ingle launch), c (per chunk), g (segments)
    int sequential_chunks;
};

static int launch_rule() {
    const std::vector<int64_t> hyb_cb = {0, 465, 945, 4785, 7000, 9000};
    const RuleCase cases[] = {
        {"persistent_nk3", true, false, false, {0, 64, 128, 200}, 0, "snn", 3},
        {"per_chunk_nk2", false, false, false, {0, 64, 100}, 0, "cc", 2},
        {"plain_split_nk1", false, true, false, {0, 1600}, 0, "g", 1},
        {"host_fed_split_nk2", false, true, false, {0, 96, 2200}, 0, "ng", 2},
        {"hybrid_persistent", true, true, true, hyb_cb, 4784, "snnnn", 3},
        {"hybrid_per_chunk", false, true, true, hyb_cb, 4784, "cccnn", 3},
        {"hybrid_step_on_a_boundary", false, true, true, hyb_cb, 4785, "ccccn", 4},
    };
    int bad = 0;
    std::printf("[");
    for (const RuleCase &c : cases) {
        PassPlan m;
        m.persistent = c.persistent; m.tsplit = c.tsplit; m.hybrid = c.hybrid; m.cb = c.cb; m.hyb_S = c.hyb_S;
        std::string got;
        for (int k = 0; k < m.nk(); ++k) got += "nscg"[(int)m.viterbi_behind(k)];
        if (got != c.behind || m.sequential_chunks() != c.sequential_chunks) ++bad;
        std::printf("%s\n{\"name\": \"%s\", \"behind\": \"%s\", \"sequential_chunks\": %d}", &c == cases ? "" : ",", c.name, got.c_str(),
                    m.sequential_chunks());
    }
    std::printf("\n]\n");
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "launch_rule")) return launch_rule();
    std::printf("[");
    for (int a = 1; a < argc; ++a) {
        std::vector<long long> v;
        for (char *tok = std::strtok(argv[a], ","); tok; tok = std::strtok(nullptr, ",")) v.push_back(std::atoll(tok));
        if (v.size() != 20) { std::fprintf(stderr, "argument %d: 20 numbers expected, got %zu\n", a, v.size()); return 2; }
        PassGeometry g;
        g.F = v[0]; g.S = v[1]; g.cmap_rows = v[2]; g.clips = v[3];
        g.lag_stride = v[4]; g.yin_stride = v[5]; g.obs_stride = v[6]; g.n_mels = v[7];
        g.pyin = v[8] != 0; g.mel = v[9] != 0; g.debug_stages = v[10] != 0; g.proportional = v[11] != 0; g.tsplit = v[12] != 0;
        g.nk = v[13]; g.n_seg = v[14]; g.tube_cap = v[15]; g.tube_record_ints = v[16]; g.seg64_size = v[17]; g.seg32_size = v[18];
        const PassBytes b = pass_bytes(g);
        const SegLayout L((size_t)v[14], (size_t)v[3], (size_t)v[19]);
        std::printf("%s\n{\"bytes\": {", a > 1 ? "," : "");
#define B(name) std::printf("\"" #name "\": %zu%s", b.name, ", ")
        B(dfn); B(logobs); B(logunv); B(obs_seg); B(ptr); B(cmap); B(bnd); B(states); B(melpow); B(clipmax); B(rake_raw); B(vstate);
        B(sample_off); B(sample_len); B(out_off); B(frame_off); B(order); B(chunk_off); B(sel_off);
        B(yin); B(chunk_lo); B(chunk_flag); B(clip_tb);
        B(seg64); B(seg32); B(seg_col); B(seg_map); B(seg_i32); B(colhist); B(colG); B(colkg); B(clip_flag); B(flag_order);
        B(tube_buf); B(tube_at);
#undef B
        std::printf("\"tube_count\": %zu}, \"layout\": {", b.tube_count);
#define O(name) std::printf("\"" #name "\": %zu, ", L.name)
        O(f0); O(ch0); O(vf_off); O(n64);
        O(T); O(store); O(prev); O(clip); O(clip_seg0); O(seg_order); O(lock_order); O(n32);
        O(kg); O(lock); O(end); O(clip_first); O(clip_dirty);
#undef O
        std::printf("\"n_i32\": %zu}}", L.n_i32);
    }
    std::printf("\n]\n");
    return 0;
}
