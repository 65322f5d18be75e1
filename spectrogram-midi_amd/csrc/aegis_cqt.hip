// Constant-Q entries of libaegis_hip.so (aegis_cqt, aegis_chroma_cqt, aegis_cqt_device) and aegis_rake_patterns.
#include "aegis_internal.h"

#include <chrono>

using namespace aegis;

extern "C" {

int aegis_rake_patterns(aegis_handle *h, const float *S_dB, int32_t n_mels, int64_t n_frames,
                        double broadband_threshold_ratio, uint8_t *mask_out) {
    ENTRY(h)
    if (n_mels <= 0 || n_frames < 0 || (n_frames > 0 && (!S_dB || !mask_out))) { h->err = "bad argument"; return AEGIS_ERR_INVALID; }
    if (n_frames == 0) return AEGIS_OK;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t img = (size_t)n_mels * n_frames * 4;
    ENSURE(h, io_sdb, img); ENSURE(h, rk_raw, n_frames); ENSURE(h, io_rake, n_frames);
    hipStream_t s = h->stream;
    StreamScope scope(h);
    HIPCHK(h, hipMemcpyAsync(h->io_sdb.p, S_dB, img, hipMemcpyHostToDevice, s));
    const RakeBounds rb = rake_frame_bounds(h->tab);
    launch_rake_from_db(h->io_sdb.as<const float>(), n_mels, n_frames, broadband_threshold_ratio,
                        rb.min_frames, rb.max_frames, h->rk_raw.as<uint8_t>(),
                        h->io_rake.as<uint8_t>(), s);
    HIPCHK(h, hipGetLastError());
    FETCH(h, mask_out, h->io_rake.p, n_frames, s);
    return scope.finish();
    ENTRY_END(h)
}

// Frees the least recently used banks until at most `keep` are left.  A kernel enqueued by an earlier call (on the handle's
// stream, or on a caller's with sync == 0) may still read a bank: the device is synchronised before the first one goes.
static int cqt_evict_locked(aegis_handle *h, size_t keep) {
    if (h->cqt_banks.size() <= keep) return AEGIS_OK;
    HIPCHK(h, hipDeviceSynchronize());
    while (h->cqt_banks.size() > keep) {
        if (h->cqt_banks.back().bank.dev) (void)hipFree(h->cqt_banks.back().bank.dev);
        h->cqt_banks.pop_back();
    }
    return AEGIS_OK;
}

// The bank of (n_bins, bins_per_octave, fmin, filter_scale) at the front of h->cqt_banks: found among the banks built so
// far, or built on the host and uploaded (the least recently used one leaves when the cache is full).  A refused bank
// touches nothing.
static int cqt_bank_locked(aegis_handle *h, int32_t &n_bins, int32_t &bins_per_octave, double &fmin, double &filter_scale, hipStream_t s) {
    if (n_bins == 0) n_bins = 84;
    if (bins_per_octave == 0) bins_per_octave = 12;
    if (!(fmin > 0)) fmin = 32.70319566257483;            // note_to_hz('C1')
    if (!(filter_scale > 0)) filter_scale = 1.0;
    auto &banks = h->cqt_banks;
    for (auto it = banks.begin(); it != banks.end(); ++it) {
        const CqtBank &b = it->bank;
        if (b.n_bins == n_bins && b.bins_per_octave == bins_per_octave && b.fmin == fmin && b.filter_scale == filter_scale && b.dev) {
            banks.splice(banks.begin(), banks, it);
            return AEGIS_OK;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    aegis_handle::CachedBank nb;
    const char *msg = build_cqt_bank(nb.bank, h->tab.sr, n_bins, fmin, bins_per_octave, filter_scale);
    if (msg[0]) { h->err = msg; return AEGIS_ERR_INVALID; }
    int rc;
    if ((rc = cqt_evict_locked(h, (size_t)h->cqt_bank_cap - 1)) != AEGIS_OK) return rc;
    // + 64 KiB: the slide kernel refills a tile's register queue unconditionally, so a wave's last groups request up to
    // kSlotDepth KiB past its stream (never used)
    nb.bytes = nb.bank.data.size() * 4 + 65536;
    auto alloc = [&]() -> hipError_t {
        if (h->fail_allocs > 0) { --h->fail_allocs; return hipErrorOutOfMemory; }      // test hook, as in grow_buf
        return hipMalloc(reinterpret_cast<void **>(&nb.bank.dev), nb.bytes);
    };
    hipError_t e = alloc();
    if (e != hipSuccess) {                                 // make room: every other bank goes, then one more try
        (void)hipGetLastError();
        nb.bank.dev = nullptr;
        if ((rc = cqt_evict_locked(h, 0)) != AEGIS_OK) return rc;
        e = alloc();
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->err = "hipMalloc(" + std::to_string(nb.bytes) + " bytes) for a CQT filter bank: " + hipGetErrorString(e);
        return AEGIS_ERR_NOMEM;
    }
    hipError_t up = hipMemset(reinterpret_cast<char *>(nb.bank.dev) + nb.bank.data.size() * 4, 0, 65536);
    if (up == hipSuccess) up = hipMemcpy(nb.bank.dev, nb.bank.data.data(), nb.bank.data.size() * 4, hipMemcpyHostToDevice);
    if (up != hipSuccess) {
        (void)hipFree(nb.bank.dev);
        h->err = std::string("upload of a CQT filter bank: ") + hipGetErrorString(up);
        return AEGIS_ERR_DEVICE;
    }
    std::vector<float>().swap(nb.bank.data);               // the kernels read the device copy only
    banks.push_front(std::move(nb));
    ++h->cqt_bank_builds;
    h->cqt_bank_bytes = (int64_t)banks.front().bytes;
    h->cqt_bank_build_us = (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    (void)s;
    return AEGIS_OK;
}

// clip geometry on the device + the launch; d_pcm and d_out are device pointers
static int cqt_launch_locked(aegis_handle *h, const float *d_pcm, const int64_t *soff, int32_t n_clips, float *d_out, hipStream_t s,
                             int64_t *total_frames) {
    std::vector<int64_t> foff(n_clips + 1, 0), toff(n_clips + 1, 0);
    for (int i = 0; i < n_clips; ++i) {
        const int64_t n = soff[i + 1] - soff[i];
        if (n < 0) { h->err = "sample_offsets must be non-decreasing"; return AEGIS_ERR_INVALID; }
        foff[i + 1] = foff[i] + 1 + n / h->tab.hop;
        toff[i + 1] = toff[i] + (1 + n / h->tab.hop + kCqtSlideFrames - 1) / kCqtSlideFrames;
    }
    ENSURE(h, q_soff, (n_clips + 1) * 8);
    {   // foff and toff (and the caller's soff) leave with this frame: a scope of their own, drained before the launch
        StreamScope geometry(h, s);
        HIPCHK(h, hipMemcpyAsync(h->q_soff.p, soff, (n_clips + 1) * 8, hipMemcpyHostToDevice, s));
        PUT(h, q_foff, foff, s); PUT(h, q_toff, toff, s);
        const int rc = geometry.finish();
        if (rc != AEGIS_OK) return rc;
    }
    CqtArgs a{d_pcm, h->q_soff.as<const int64_t>(), h->q_foff.as<const int64_t>(), n_clips,
              foff[n_clips], h->tab.hop, d_out};
    drop_events(h);
    TIMED(h, "cqt", s, launch_cqt(a, h->cqt_banks.front().bank, h->q_toff.as<const int64_t>(), toff[n_clips], s));
    *total_frames = foff[n_clips];
    return AEGIS_OK;
}

// What the two host-buffer entries share (handle locked, device set): the bank, the clips validated and packed, the staging
// sized, the samples uploaded (behind the chroma fold's bin classes, when there are any), the CQT launched into q_out.
// F: frames of all clips.
// (declared in aegis_internal.h with C++ linkage: aegis_salience.hip runs it in front of its kernel)
}  // extern "C"
int aegis::cqt_host_locked(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips, int32_t &n_bins,
                           int32_t bins_per_octave, double fmin, double filter_scale, int32_t n_chroma, const int32_t *bin_class, int64_t *F_out) {
    hipStream_t s = h->stream;
    int rc;
    if ((rc = cqt_bank_locked(h, n_bins, bins_per_octave, fmin, filter_scale, s)) != AEGIS_OK) return rc;
    for (int b = 0; bin_class && b < n_bins; ++b)
        if (bin_class[b] < 0 || bin_class[b] >= n_chroma) { h->err = "bin_class entries must lie in [0, n_chroma)"; return AEGIS_ERR_INVALID; }
    std::vector<int64_t> soff;
    if ((rc = clip_samples(h, "", pcm, n_samples, 0, n_clips, soff)) != AEGIS_OK) return rc;
    int64_t F = 0;
    for (int i = 0; i < n_clips; ++i) F += 1 + n_samples[i] / h->tab.hop;
    ENSURE(h, q_out, (size_t)F * n_bins * 4);
    if (bin_class) {
        ENSURE(h, q_chroma, (size_t)F * n_chroma * 4); ENSURE(h, q_cls, (size_t)n_bins * 4);
        HIPCHK(h, hipMemcpyAsync(h->q_cls.p, bin_class, (size_t)n_bins * 4, hipMemcpyHostToDevice, s));
    }
    if ((rc = upload_clips(h, h->q_pcm, pcm, 0, soff, s)) != AEGIS_OK) return rc;
    int64_t Fd = 0;
    *F_out = F;
    return cqt_launch_locked(h, h->q_pcm.as<const float>(), soff.data(), n_clips, h->q_out.as<float>(), s, &Fd);
}
extern "C" {

int aegis_cqt(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
              int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, float *mag_out) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !mag_out))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    int64_t F = 0;
    StreamScope scope(h);
    const int rc = cqt_host_locked(h, pcm, n_samples, n_clips, n_bins, bins_per_octave, fmin, filter_scale, 0, nullptr, &F);
    if (rc != AEGIS_OK) return rc;
    FETCH(h, mag_out, h->q_out.p, F * n_bins, h->stream);
    return scope.finish();
    ENTRY_END(h)
}

int aegis_chroma_cqt(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                     int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, int32_t n_chroma,
                     const int32_t *bin_class, float *chroma_out) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !chroma_out)) || !bin_class) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    if (n_chroma < 1 || n_chroma > 24) { h->err = "n_chroma must be 1..24"; return AEGIS_ERR_INVALID; }
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int64_t F = 0;
    StreamScope scope(h);
    const int rc = cqt_host_locked(h, pcm, n_samples, n_clips, n_bins, bins_per_octave, fmin, filter_scale, n_chroma, bin_class, &F);
    if (rc != AEGIS_OK) return rc;
    TIMED(h, "chroma", s, launch_chroma_fold(h->q_out.as<const float>(), h->q_foff.as<const int64_t>(), n_clips, F, n_bins, n_chroma,
                                             h->q_cls.as<const int32_t>(), h->q_chroma.as<float>(), s));
    FETCH(h, chroma_out, h->q_chroma.p, F * n_chroma, s);
    return scope.finish();
    ENTRY_END(h)
}

int aegis_cqt_device(aegis_handle *h, const float *d_pcm, const int64_t *sample_offsets, int32_t n_clips,
                     int32_t n_bins, int32_t bins_per_octave, double fmin, double filter_scale, float *d_mag_out,
                     void *stream, int32_t sync) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && (!sample_offsets || !d_mag_out))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    DEVICE_ONLY(h);
    if (sample_offsets[n_clips] > sample_offsets[0] && !d_pcm) { h->err = "d_pcm == NULL"; return AEGIS_ERR_INVALID; }
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    int rc;
    StreamScope scope(h, s);
    if ((rc = cqt_bank_locked(h, n_bins, bins_per_octave, fmin, filter_scale, s)) != AEGIS_OK) return rc;
    int64_t F = 0;
    if ((rc = cqt_launch_locked(h, d_pcm, sample_offsets, n_clips, d_mag_out, s, &F)) != AEGIS_OK) return rc;
    if (sync) return scope.finish();
    scope.leave_enqueued();
    return AEGIS_OK;
    ENTRY_END(h)
}

/* see include/aegis_hip.h */
int aegis_estimate_tuning(aegis_handle *h, const float *const *pcm, const int64_t *n_samples, int32_t n_clips,
                          int32_t bins_per_octave, double *tuning_out, int32_t *counts_out, int64_t *n_peaks_out) {
    ENTRY(h)
    if (n_clips < 0 || (n_clips > 0 && (!pcm || !n_samples || !tuning_out))) { h->err = "null argument"; return AEGIS_ERR_INVALID; }
    if (bins_per_octave < 1) { h->err = "bins_per_octave must be positive"; return AEGIS_ERR_INVALID; }
    if (h->tab.n_fft != kTunFft) { h->err = "estimate_tuning: only n_fft = 2048 is built (the twiddle and window tables are the handle's)"; return AEGIS_ERR_INVALID; }
    if (n_clips == 0) return AEGIS_OK;
    DEVICE_ONLY(h);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->tn_last_peak_off.clear();                               // a call that fails below leaves nothing to fetch
    TuningArgs a{};
    a.sr = h->tab.sr; a.bpo = bins_per_octave; a.n_clips = n_clips;
    tuning_band(a.sr, &a.k_lo, &a.k_hi);
    const int64_t per_frame = (a.k_hi - a.k_lo + 1) / 2;       // two adjacent bins cannot both be peaks
    // geometry: [sample_off | frame_off | peak_off], n_clips + 1 entries each
    const size_t m = (size_t)n_clips + 1;
    std::vector<int64_t> soff, geo(3 * m, 0);
    int rc = clip_samples(h, "", pcm, n_samples, 0, n_clips, soff);
    if (rc != AEGIS_OK) return rc;
    std::copy(soff.begin(), soff.end(), geo.begin());
    int64_t *foff = geo.data() + m, *poff = foff + m;
    for (int i = 0; i < n_clips; ++i) {
        const int64_t frames = 1 + n_samples[i] / kTunHop;
        foff[i + 1] = foff[i] + frames;
        poff[i + 1] = poff[i] + frames * per_frame;
    }
    if (foff[n_clips] >= ((int64_t)1 << 31)) { h->err = "estimate_tuning: too many frames for one call"; return AEGIS_ERR_INVALID; }
    std::vector<unsigned long long> np_host(n_peaks_out ? (size_t)n_clips : 0);
    const size_t peaks = (size_t)std::max<int64_t>(poff[n_clips], 1);
    ENSURE(h, tn_pitch, peaks * 4); ENSURE(h, tn_mag, peaks * 4); ENSURE(h, tn_count, (size_t)n_clips * 8);
    ENSURE(h, tn_median, (size_t)n_clips * 4); ENSURE(h, tn_cells, (size_t)n_clips * kTunCells * 4); ENSURE(h, tn_tuning, (size_t)n_clips * 8);
    StreamScope scope(h);
    PUT(h, tn_meta, geo, s);
    HIPCHK(h, hipMemsetAsync(h->tn_count.p, 0, (size_t)n_clips * 8, s));
    if ((rc = upload_clips(h, h->q_pcm, pcm, 0, soff, s)) != AEGIS_OK) return rc;
    a.pcm = h->q_pcm.as<const float>();
    a.sample_off = h->tn_meta.as<const int64_t>();
    a.frame_off = a.sample_off + m;
    a.peak_off = a.frame_off + m;
    a.n_frames = foff[n_clips];
    a.hann = h->dt.hann; a.twiddle = h->dt.twiddle; a.edges = h->d_tuning_edges;
    a.pitch = h->tn_pitch.as<float>(); a.mag = h->tn_mag.as<float>();
    a.n_peaks = h->tn_count.as<unsigned long long>();
    a.median = h->tn_median.as<float>();
    a.counts = h->tn_cells.as<int32_t>();
    a.tuning = h->tn_tuning.as<double>();
    drop_events(h);
    TIMED(h, "tuning_peaks", s, launch_tuning_peaks(a, s));
    TIMED(h, "tuning_select", s, launch_tuning_select(a, s));
    TIMED(h, "tuning_hist", s, launch_tuning_hist(a, s));
    FETCH(h, tuning_out, h->tn_tuning.p, n_clips, s);
    if (counts_out) FETCH(h, counts_out, h->tn_cells.p, (size_t)n_clips * kTunCells, s);
    if (n_peaks_out) FETCH(h, np_host.data(), h->tn_count.p, n_clips, s);
    if ((rc = scope.finish()) != AEGIS_OK) return rc;
    for (size_t i = 0; i < np_host.size(); ++i) n_peaks_out[i] = (int64_t)np_host[i];
    h->tn_last_peak_off.assign(poff, poff + m);
    return AEGIS_OK;
    ENTRY_END(h)
}

}  // extern "C"
