"""Compile-only guard of the overlap-save kernel's steady-state loop (libtsd_amd/csrc/ols.hip, ols_body).

The FIR headline runs at the speed of that loop's memory skeleton: each interior block issues the next block's loads
before its forward transform, waits for them after its inverse transform, then issues its own stores and moves on.  The
loop overlaps memory with compute only if hipcc places no `s_waitcnt vmcnt` between
  * a block's stores and the next prefetch's loads (a wait there drains the stores before the prefetch is issued), and
  * the prefetch's loads and the transform they hide under (a wait there exposes the load latency).
Small source changes (a predicate around the loads or the wait, a pull of the work counter after the stores) have put
such waits back in before, so this test reads the gfx950 assembly of the R0 = 2, dynamic hand-out kernels (the ones
the 127-tap benchmark runs) and checks both properties, plus 0 scratch, <= 256 VGPRs and 2 waves per SIMD.

It anchors on groups of global loads / stores and on the first LDS write after a load group -- not on line numbers or
labels -- so that unrelated codegen churn does not break it.  Skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libtsd_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if not os.path.exists(HIPCC):
    HIPCC = shutil.which("hipcc") or HIPCC

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# ols_kernel<REAL, R0 = 2, DYN = true>; fewest loads / stores of an interior block (complex: the 14 rows past the 2 overlap
# rows, dwordx2 each; real: twice as many dword accesses)
KERNELS = {
    "complex": ("_ZN6tsdgpu10ols_kernelILb0ELi2ELb1EEEv", 14),
    "real": ("_ZN6tsdgpu10ols_kernelILb1ELi2ELb1EEEv", 28),
}


def _makefile_flags():
    """HIPFLAGS of the Makefile for ols.o: the common line plus the per-object additions."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    base = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)
    extra = " ".join(re.findall(r"^build/ols\.o:\s*HIPFLAGS\s*\+=\s*(.*)$", mk, re.M))
    flags = (base + " " + extra).replace("$(ARCH)", arch).replace("$(EXTRA)", "")
    return flags.split()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("ols_isa")
    asm = out / "ols.s"
    cmd = [HIPCC] + _makefile_flags() + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                         os.path.join(CSRC, "ols.hip"), "-o", str(asm)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(out))
    assert r.returncode == 0, r.stderr[-4000:]
    return asm.read_text(), r.stderr


def _body(text, sym):
    start = text.index("\n" + sym)
    start = text.index(":", start) + 1
    end = text.index(".Lfunc_end", start)
    return text[start:end]


def _tokens(body):
    """(kind, text) per instruction or label: load / store / vmwait / ds / label / branch / endpgm / other."""
    toks = []
    for line in body.splitlines():
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        if t.endswith(":"):
            toks.append(("label", t[:-1]))
            continue
        op = t.split()[0]
        if op.startswith("global_load_") or op.startswith("buffer_load_"):
            toks.append(("load", t))
        elif op.startswith("global_store_") or op.startswith("buffer_store_"):
            toks.append(("store", t))
        elif op == "s_waitcnt" and "vmcnt" in t:
            toks.append(("vmwait", t))
        elif op.startswith("ds_write"):
            toks.append(("dsw", t))
        elif op.startswith("ds_"):
            toks.append(("ds", t))
        elif op == "s_branch":
            toks.append(("branch", t.split()[1]))
        elif op.startswith("s_cbranch_"):
            toks.append(("cbranch", t.split()[1]))
        elif op == "s_endpgm":
            toks.append(("endpgm", t))
        else:
            toks.append(("other", t))
    return toks


def _groups(toks, kind, min_size):
    """[first, last] token indices of the runs of `kind` with nothing but ALU work, labels and branches between their
    members (no other memory access, no vmcnt wait), of at least min_size instructions."""
    out, cur = [], []
    stop = {"load", "store", "vmwait", "dsw", "ds"} - {kind}
    for i, (k, _) in enumerate(toks):
        if k == kind:
            cur.append(i)
        elif k in stop:
            if len(cur) >= min_size:
                out.append((cur[0], cur[-1]))
            cur = []
    if len(cur) >= min_size:
        out.append((cur[0], cur[-1]))
    return out


def _main_loop(toks):
    """[first, last] token indices of the steady-state loop: of the backward branches, the one whose span holds the most
    stores (the edge blocks and the history wave of the same kernel run straight-line code outside it)."""
    labels = {t: i for i, (k, t) in enumerate(toks) if k == "label"}
    best, span = 0, None
    for i, (k, t) in enumerate(toks):
        if k in ("branch", "cbranch") and t in labels and labels[t] < i:
            n = sum(1 for j in range(labels[t], i) if toks[j][0] == "store")
            if n > best:
                best, span = n, (labels[t], i)
    return span


def _waits_after_stores(toks, stores, loads):
    """For every store group: the vmcnt waits met on the fall-through path (following unconditional branches) before the
    next prefetch group begins."""
    labels = {t: i for i, (k, t) in enumerate(toks) if k == "label"}
    found = []
    for _, last in stores:
        i, jumps, waits = last + 1, 0, []
        while i < len(toks):
            k, t = toks[i]
            if k == "endpgm" or any(a <= i <= b for a, b in loads):     # (a branch may enter the group past its first load)
                break
            if k == "vmwait":
                waits.append(t)
            if k == "branch" and t in labels and jumps < 16:
                i, jumps = labels[t], jumps + 1
                continue
            i += 1
        found.append(waits)
    return found


def _waits_before_transform(toks, loads):
    """For every prefetch group that the next LDS write follows without another big load group in between: the vmcnt
    waits between its last load and that write (the head of the forward transform)."""
    found = []
    for n, (_, last) in enumerate(loads):
        nxt = loads[n + 1][0] if n + 1 < len(loads) else len(toks)
        waits = []
        for i in range(last + 1, nxt):
            k, t = toks[i]
            if k == "vmwait":
                waits.append(t)
            if k == "dsw":
                found.append(waits)
                break
            if k == "load":        # a small (guarded) load: not the prefetch this group hides
                break
    return found


@pytest.mark.parametrize("flavour", sorted(KERNELS))
def test_steady_state_loop_overlaps(isa, flavour):
    text, _ = isa
    sym, per_block = KERNELS[flavour]
    toks = _tokens(_body(text, sym))
    loop = _main_loop(toks)
    assert loop, f"{flavour}: no loop with stores found"
    inside = lambda g: loop[0] <= g[0] and g[1] <= loop[1]
    loads = [g for g in _groups(toks, "load", per_block) if inside(g)]
    stores = [g for g in _groups(toks, "store", per_block) if inside(g)]
    # the loop is unrolled twice (process(A, B), process(B, A)): at least two prefetch and two store groups
    assert len(stores) >= 2, f"{flavour}: {len(stores)} store groups of >= {per_block}"
    heads = _waits_before_transform(toks, loads)
    assert len(heads) >= 2, f"{flavour}: {len(heads)} prefetch groups followed by a transform"
    for waits in heads:
        assert not waits, f"{flavour}: the transform waits for the prefetch it should hide: {waits}"
    for waits in _waits_after_stores(toks, stores, loads):
        assert not waits, f"{flavour}: stores drained before the next prefetch: {waits}"


def test_resources(isa):
    _, remarks = isa
    for flavour, (sym, _) in KERNELS.items():
        m = re.search(re.escape(sym) + r".*?\n(.*?)LDS Size", remarks, re.S)
        assert m, f"no resource remark for {flavour}"
        block = m.group(1)
        vgpr = int(re.search(r"VGPRs: (\d+)", block).group(1))
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block).group(1))
        assert scratch == 0, f"{flavour}: {scratch} B of scratch per lane"
        assert vgpr <= 256, f"{flavour}: {vgpr} VGPRs"
        assert occ >= 2, f"{flavour}: {occ} waves per SIMD"
