"""Static instruction account of k_substep_blocked, phase by phase, from hipcc's assembly: the substep loop (beam phase, particle
phase) and what runs once per launch around it (prologue, the two rounds of requests, fix-ups and LDS fill, store phase).

A scratch copy of sb_blocked.hip gets empty `asm volatile` comment markers around the beam phase (and in front of every entry
group) and around the particle phase (and in front of every particle slot); it is compiled for gfx950 with the library's flags
(-S --offload-device-only) and the instructions of one variant are counted between the markers, in the order of the text.
The counts are STATIC: both sides of a branch count where the compiler laid them out, and the scheduler may move an
instruction across a marker (a comment is no barrier), so a slot's figure is good to a few instructions; the phase totals,
which end at barriers, are exact.  Nothing in the tree is changed.

The once-per-launch regions are cut where the source's phases begin; `fixup_fill` ends at the barrier in front of the loop, and what
lies between that barrier and the loop's first marker (rest-length targets, the first prefixes) is `loop_head`.
--root names another checkout of the repository to account (the parent commit's, to set two tables side by side): the anchors are
text both have.  The default variant is the headline's, with the addressing argument where the source has one: flat, or the buffer
form under EXTRA=-DSB_BK_BUFFER=1 (the library instantiates it only then).

Usage: python tools/phase_isa.py [--root DIR] [--variant "2, false, true, false, true, true"] [--keep file.s] [--dump-slot N]"""
import argparse, collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
CSRC = os.path.join(ROOT, "softbody-webgpu_amd", "csrc")
def library_flags():
    """HIPFLAGS of csrc/Makefile, the flags the library is built with (continuation lines joined, $(ARCH) filled in)."""
    mk = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*\?=\s*(.*)$", mk, re.M)}
    if "HIPFLAGS" not in var:
        sys.exit("no HIPFLAGS in csrc/Makefile: update tools/phase_isa.py")
    return [f for f in re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["HIPFLAGS"]).split() if not f.startswith("-W")]


FLAGS = library_flags()
MARK = 'asm volatile("; SBMARK %s");'
# (anchor text in sb_blocked.hip, marker, before or after the anchor)
ANCHORS = [
    ("    float moved_sum = 0.0f; // TRACK", "prologue", "before"),
    ("    const uint32_t nh_load = np_load - n_own, nh_move = np_move - n_own,", "request1", "before"),
    ("    // (2) the gathers\n", "request2", "before"),
    ("    // (what the lanes with nothing to fetch hold instead", "fixup_fill", "before"),
    ("    // targets nobody fetched (tiles that have never yielded", "loop_head", "before"),
    ("    uint32_t tid_s = tid;\n", "store", "before"),
    ("#pragma unroll\n        for (int i0 = 0; i0 < SB_BK_MAXB; i0 += SB_BK_G) {", "beam_begin", "before"),
    ("            const uint32_t j0 = SB_ENT_J(i0);\n", "beam_group", "before"),
    ("        if (!(SB_BK_ABLATE & 32)) __syncthreads();\n        // ---- particle phase", "beam_end", "before"),
    ("        float moved_now = 0.0f;\n", "particle_begin", "after"),
    ("            const uint32_t q = SB_SLOT_Q(i);\n            if (i < (int)SB_BK_OWNP ? q < n_own : q < npr)", "particle_slot", "before"),
    ("        if (TRACK) moved_sum += moved_now;\n", "particle_end", "before"),
]
QUARTER = ("v_rsq_", "v_rcp_", "v_sqrt_", "v_cvt_", "v_exp_", "v_log_", "v_sin_", "v_cos_")


def marked_source():
    src = open(os.path.join(CSRC, "sb_blocked.hip")).read()
    for text, name, where in ANCHORS:
        if src.count(text) != 1:
            sys.exit("anchor for %s found %d times in sb_blocked.hip: update tools/phase_isa.py" % (name, src.count(text)))
        src = src.replace(text, MARK % name + "\n" + text if where == "before" else text + MARK % name + "\n")
    return src


def compile_asm(keep):
    with tempfile.TemporaryDirectory() as d:
        cs = os.path.join(d, "a", "csrc")  # (sb_engine.h includes ../../include/softbody.h)
        os.makedirs(cs)
        os.makedirs(os.path.join(d, "include"))
        for f in os.listdir(CSRC):
            if f.endswith(".h"):
                open(os.path.join(cs, f), "w").write(open(os.path.join(CSRC, f)).read())
        open(os.path.join(d, "include", "softbody.h"), "w").write(open(os.path.join(ROOT, "include", "softbody.h")).read())
        open(os.path.join(cs, "sb_blocked.hip"), "w").write(marked_source())
        out = os.path.join(d, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *os.environ.get("EXTRA", "").split(), "-S", "--offload-device-only",
                        os.path.join(cs, "sb_blocked.hip"), "-o", out], check=True)
        text = open(out).read()
    if keep:
        open(keep, "w").write(text)
    return text


def kernel_body(text, variant):
    want = "k_substep_blocked<%s>" % variant
    lines = text.split("\n")
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w*k_substep_blocked\w*):", l)
        if not m:
            continue
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout
        if want in name:
            j = i
            while not lines[j].startswith("\t.end_amdhsa_kernel") and not lines[j].startswith(".Lfunc_end"):
                j += 1
            return lines[i:j]
    sys.exit("no kernel %s in the assembly" % want)


def is_instr(l):
    s = l.strip()
    return l.startswith("\t") and s and not s.startswith((".", ";"))


def classify(l):
    op = l.strip().split()[0]
    k = []
    if op.startswith("v_"):  # (v_readlane / v_readfirstlane included: SQ_INSTS_VALU counts them too)
        k.append("valu")
        if op.startswith(QUARTER):
            k.append("quarter")
        if op.startswith(("v_cmp", "v_cmpx")):
            k.append("vcmp")
    if op.startswith("ds_"):
        k.append("lds")
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        k.append("vmem")
    if op.startswith("s_waitcnt"):
        k.append("waitcnt")
    if op in ("s_cbranch_execz", "s_cbranch_execnz") or op.startswith(("s_and_saveexec", "s_or_saveexec", "s_xor_saveexec")):
        k.append("exec_branch" if op.startswith("s_cbranch") else "saveexec")
    if op.startswith("s_cbranch_vcc") or op.startswith("s_cbranch_scc"):
        k.append("uniform_branch")
    if op.startswith("s_") and not k:
        k.append("salu")
    k.append("all")
    return k


def account(body):
    regions, cur, seq = [], None, collections.Counter()
    for l in body:
        m = re.search(r"; SBMARK (\w+)", l)
        if m:
            name = m.group(1)
            seq[name] += 1
            cur = {"name": "%s[%d]" % (name, seq[name] - 1) if name in ("beam_group", "particle_slot") else name, "lines": []}
            regions.append(cur)
        elif cur is not None and is_instr(l):
            cur["lines"].append(l)
    return regions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", help="another checkout of the repository (read at import)")
    ap.add_argument("--variant", default="2, false, true, false, true" + ((", true" if "SB_BK_BUFFER=1" in os.environ.get("EXTRA", "") else ", false")
                                                                        if "bool BUF" in open(os.path.join(CSRC, "sb_blocked.hip")).read() else ""))
    ap.add_argument("--keep")
    ap.add_argument("--dump-slot", type=int, default=-1, help="print the instructions of this particle slot")
    a = ap.parse_args()
    regions = account(kernel_body(compile_asm(a.keep), a.variant))
    cols = ["all", "valu", "quarter", "vcmp", "lds", "vmem", "waitcnt", "saveexec", "exec_branch", "uniform_branch", "salu"]
    ONCE = ("prologue", "request1", "request2", "fixup_fill", "loop_head", "store")
    print("k_substep_blocked<%s>: static instructions of one substep iteration, by marker region" % a.variant)
    print("%-18s" % "region" + "".join("%9s" % c[:8] for c in cols))
    tot = collections.defaultdict(collections.Counter)
    for r in regions:
        if r["name"] in ("beam_end", "particle_end") or r["name"] in ONCE:
            continue  # (what follows these is the barrier and the loop's tail)
        c = collections.Counter(k for l in r["lines"] for k in classify(l))
        phase = "beam" if r["name"].startswith("beam") else "particle"
        tot[phase].update(c)
        print("%-18s" % r["name"] + "".join("%9d" % c[k] for k in cols))
    for ph in ("beam", "particle"):
        print("%-18s" % (ph + " phase") + "".join("%9d" % tot[ph][k] for k in cols))
    v = tot["beam"]["valu"] + tot["particle"]["valu"]
    print("particle phase: %.1f %% of the loop's static VALU instructions (%d of %d)" % (100.0 * tot["particle"]["valu"] / v, tot["particle"]["valu"], v))
    print()
    print("k_substep_blocked<%s>: static instructions per thread that run once per launch, by marker region" % a.variant)
    print("%-18s" % "region" + "".join("%9s" % c[:8] for c in cols))
    once = collections.Counter()
    for r in regions:
        if r["name"] in ONCE:
            c = collections.Counter(k for l in r["lines"] for k in classify(l))
            once.update(c)
            print("%-18s" % r["name"] + "".join("%9d" % c[k] for k in cols))
    print("%-18s" % "once per launch" + "".join("%9d" % once[k] for k in cols))
    if a.dump_slot >= 0:
        for r in regions:
            if r["name"] == "particle_slot[%d]" % a.dump_slot:
                print("\n".join(r["lines"]))


if __name__ == "__main__":
    main()
