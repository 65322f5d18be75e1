"""How many memory requests a kernel keeps in flight, read from its gfx950 assembly.

    python tools/isa_inflight.py spectrogram-midi_amd/csrc/frame.hip [--kernel frame_yin_kernelILb0E] [--json]

The file is cross-compiled device-only to assembly with the flags of csrc/Makefile (no GPU needed), the named kernel is cut at
its `s_barrier`s, and per region (numbered in program order, region 0 runs up to the first barrier) the tool prints

    LDS reads, and the `(in flight -> waited down to)` pair of every `s_waitcnt lgkmcnt(N)`,
    global loads, and the same pairs for `s_waitcnt vmcnt(N)`,
    `single`: the number of waits at zero with exactly ONE read outstanding -- a full LDS (or L2) round trip that covers
              nothing but itself, the pattern the frame kernel's mel, rms and quotient sections were rewritten to avoid,
    for every run of global loads, `cover`: how many other memory instructions stand between its last load and the first
              wait that covers the run.

A wait is a statement about a counter, and the counters count every LDS instruction (lgkmcnt) and every vector-memory
instruction, stores included (vmcnt), which return in order.  The tool therefore counts every `ds_*` towards lgkmcnt and
every `global_*` / `buffer_*` / `scratch_*` towards vmcnt, by prefix, to know what a wait at N leaves outstanding; what it
reports are the READS among them.  Scalar loads are not followed: a wait they force shows as a wait to zero, which is what
it costs.  The program is read in text order -- a region with a branch in it is taken as if both sides ran, which is how the
frame kernel's `if (has_chunk)` bodies read."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAKEFILE = os.path.join(ROOT, "spectrogram-midi_amd", "csrc", "Makefile")
HIPCC_DEFAULT = "/opt/rocm/bin/hipcc"

_WAIT_FIELD = re.compile(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)")


def find_hipcc():
    for c in (os.environ.get("HIPCC"), HIPCC_DEFAULT, shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def makefile_flags(path=MAKEFILE):
    """CXXFLAGS of the Makefile, without -fPIC (host only) and the $(EXTRA) hook."""
    with open(path) as f:
        for line in f:
            m = re.match(r"CXXFLAGS\s*=\s*(.*)$", line)
            if m:
                return [w for w in m.group(1).split() if not w.startswith("$(") and w != "-fPIC"]
    raise RuntimeError(f"no CXXFLAGS in {path}")


def compile_to_asm(hip_file, hipcc=None, arch="gfx950", extra=()):
    hipcc = hipcc or find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found")
    hip_file = os.path.abspath(hip_file)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernel.s")
        cmd = [hipcc, *makefile_flags(), *extra, f"--offload-arch={arch}", "--cuda-device-only", "-S", hip_file, "-o", out]
        subprocess.run(cmd, check=True, cwd=os.path.dirname(os.path.abspath(hip_file)))
        with open(out) as f:
            return f.read()


def kernel_span(lines, kernel):
    """(label line, end line) of the first function whose label contains `kernel`, as indices into `lines`."""
    start = None
    for i, ln in enumerate(lines):
        if start is None:
            if re.match(r"^[A-Za-z_][\w$.]*:", ln) and kernel in ln.split(":")[0]:
                start = i
        elif ln.startswith(".Lfunc_end"):
            return start, i
    raise RuntimeError(f"kernel {kernel!r} not found")


def kernel_body(asm, kernel):
    """[(line number, mnemonic, operands)] of the first function whose label contains `kernel`."""
    lines = asm.splitlines()
    start, end = kernel_span(lines, kernel)
    body = []
    for n in range(start + 1, end):
        t = lines[n].split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        parts = t.split(None, 1)
        body.append((n + 1, parts[0], parts[1] if len(parts) > 1 else ""))
    return body


def decode_wait(operands):
    """{counter: N} of an s_waitcnt, symbolic or as the raw gfx9 immediate."""
    got = {k: int(v) for k, v in _WAIT_FIELD.findall(operands)}
    if not got and re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", operands.strip()):
        imm = int(operands.strip(), 0)
        vm, lgkm = (imm & 0xF) | ((imm >> 14) & 0x3) << 4, (imm >> 8) & 0xF
        if vm != 63:
            got["vmcnt"] = vm
        if lgkm != 15:
            got["lgkmcnt"] = lgkm
    return got


def is_lds(m):
    return m.startswith("ds_")


def is_lds_read(m):
    return m.startswith("ds_read")


def is_vmem(m):
    return m.startswith(("global_", "buffer_", "scratch_"))


def is_global_load(m):
    return m.startswith(("global_load", "buffer_load"))


class _Counter:
    """One in-order counter: the outstanding instructions, oldest first; a read is (memory-instruction index, asm line)."""

    def __init__(self):
        self.q = []

    def issue(self, read):
        self.q.append(read)

    def wait(self, n):
        """Reads outstanding before, after, and the reads the wait has just covered."""
        before = sum(e is not None for e in self.q)
        done = []
        if n < len(self.q):
            done = [e for e in self.q[:len(self.q) - n] if e is not None]
            self.q = self.q[len(self.q) - n:]
        return before, sum(e is not None for e in self.q), done


def analyse(body):
    """The regions between barriers: a list of dicts (see the module docstring)."""
    regions = []

    def fresh(line):
        return dict(first_line=line, last_line=line, lds_reads=0, global_loads=0, lgkm_waits=[], vm_waits=[], lgkm_single=0,
                    vm_single=0, vm_wait_lines=[], cover=[], lds_writes_before_first_vm_wait=None)

    lgkm, vm = _Counter(), _Counter()
    cur = fresh(body[0][0] if body else 0)
    mi = 0                         # memory instructions so far
    lds_w_seen = 0
    for line, m, ops in body:
        cur["last_line"] = line
        if m == "s_barrier":
            regions.append(cur)
            cur = fresh(line)
            lds_w_seen = 0
            continue
        if m == "s_waitcnt":
            w = decode_wait(ops)
            if "lgkmcnt" in w:
                a, b, _ = lgkm.wait(w["lgkmcnt"])
                if a:
                    cur["lgkm_waits"].append((a, b))
                    cur["lgkm_single"] += (a == 1 and w["lgkmcnt"] == 0)
            if "vmcnt" in w:
                a, b, done = vm.wait(w["vmcnt"])
                cur["vm_wait_lines"].append(line)
                if cur["lds_writes_before_first_vm_wait"] is None:
                    cur["lds_writes_before_first_vm_wait"] = lds_w_seen
                if a:
                    cur["vm_waits"].append((a, b))
                    cur["vm_single"] += (a == 1 and w["vmcnt"] == 0)
                run = []                                 # loads issued back to back are one request
                for e in done + [None]:
                    if run and (e is None or e[0] != run[-1][0] + 1):
                        cur["cover"].append(dict(loads=len(run), first_load_line=run[0][1], wait_line=line,
                                                 other_memory_instructions=mi - run[-1][0]))
                        run = []
                    if e is not None:
                        run.append(e)
            continue
        if is_lds(m):
            mi += 1
            rd = is_lds_read(m)
            lgkm.issue((mi, line) if rd else None)
            cur["lds_reads"] += rd
            lds_w_seen += not rd
        elif is_vmem(m):
            mi += 1
            ld = is_global_load(m)
            vm.issue((mi, line) if ld else None)
            cur["global_loads"] += ld
    regions.append(cur)
    return regions


def loop_head(asm, kernel):
    """The loop of the kernel that holds the most barriers (the frame kernel's pair loop): the asm line of its header and
    the mnemonics of the LDS writes that follow the header, in text order, before the first `s_waitcnt` that names vmcnt
    (None: the kernel has no loop)."""
    lines = asm.splitlines()
    start, end = kernel_span(lines, kernel)
    # the compiler names every block's loop in a comment: `=>This Loop Header: Depth=1` on the header's label and
    # `in Loop: Header=BB0_231 Depth=1` (or `Parent Loop BB0_231`) on the loop's other blocks, wherever it has laid them out
    heads, owner, count = {}, None, {}
    for i in range(start, end):
        m = re.match(r"^\.L(BB\w+):(.*)$", lines[i])
        if m:
            c = m.group(2)
            if "Loop Header: Depth=1" in c:
                owner = m.group(1)
                heads[owner] = i
            else:
                o = re.search(r"(?:Header=|Parent Loop )(BB\w+)", c)
                owner = o.group(1) if o else None
        elif owner is not None and lines[i].split(";")[0].strip() == "s_barrier":
            count[owner] = count.get(owner, 0) + 1
    best = None
    for h, i in heads.items():
        if best is None or count.get(h, 0) > best[0]:
            best = (count.get(h, 0), i, end)
    if best is None:
        return None
    writes = []
    for k in range(best[1], best[2]):
        t = lines[k].split(";")[0].split(None, 1)
        if not t:
            continue
        if t[0] == "s_waitcnt" and "vmcnt" in decode_wait(t[1] if len(t) > 1 else ""):
            break
        if is_lds(t[0]) and not is_lds_read(t[0]):
            writes.append(t[0])
    return dict(header_line=best[1] + 1, barriers=best[0], lds_writes_before_first_vm_wait=writes)


def _pairs(ws):
    return " ".join(f"{a}>{b}" for a, b in ws) or "-"


def render(regions):
    out = []
    for i, r in enumerate(regions):
        out.append(f"region {i:3d}  asm {r['first_line']}-{r['last_line']}  LDS reads {r['lds_reads']:3d}  single {r['lgkm_single']:2d}  "
                   f"global loads {r['global_loads']:2d}  single {r['vm_single']}")
        if r["lgkm_waits"]:
            out.append(f"            lgkmcnt: {_pairs(r['lgkm_waits'])}")
        if r["vm_waits"]:
            out.append(f"            vmcnt:   {_pairs(r['vm_waits'])}")
        for c in r["cover"]:
            out.append(f"            {c['loads']} global load(s) from asm {c['first_load_line']}: {c['other_memory_instructions']} other memory "
                       f"instruction(s) before the wait that covers them (asm {c['wait_line']})")
    tot = sum(r["lgkm_single"] for r in regions if r["lds_reads"] >= 6)
    out.append(f"waits at lgkmcnt(0) with one read outstanding, in regions with at least six LDS reads: {tot}")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("hip_file")
    ap.add_argument("--kernel", default="frame_yin_kernelILb0E", help="substring of the kernel's (mangled) name")
    ap.add_argument("--hipcc", default=None)
    ap.add_argument("--asm", action="store_true", help="the file is assembly already: do not compile")
    ap.add_argument("--extra", action="append", default=[], help="a further compiler flag, e.g. --extra=-DAEGIS_ABLATE=128")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.asm:
        with open(a.hip_file) as f:
            asm = f.read()
    else:
        asm = compile_to_asm(a.hip_file, hipcc=a.hipcc, extra=a.extra)
    regions = analyse(kernel_body(asm, a.kernel))
    head = loop_head(asm, a.kernel)
    if a.json:
        print(json.dumps(dict(regions=regions, loop=head), indent=1))
        return
    print(render(regions))
    if head:
        print(f"loop with the most barriers ({head['barriers']}): header asm {head['header_line']}, "
              f"{len(head['lds_writes_before_first_vm_wait'])} LDS write(s) after the header before the first s_waitcnt vmcnt "
              f"({' '.join(head['lds_writes_before_first_vm_wait'])})")


if __name__ == "__main__":
    sys.exit(main())
