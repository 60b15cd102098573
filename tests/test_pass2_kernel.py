"""Pass 2 (sgp_suffstats_bwd, sgp_suffstats_bwd_factored(_ex)) and the K_uu gradient (sgp_kuu_bwd) against the long-double reference of
tests/pass2_reference.py, template instance by template instance.

The check everywhere is component-wise  |got - ref| <= TAU * A,  TAU = 1e-12, A the condition scale of the component (the same sum with
every factor replaced by its absolute value, see pass2_reference).  TAU is the tolerance the project applies to pass 1's sums
(test_gpu_parity.py); it is above the worst-case fp64 rounding (chain length) * 2^-53 of every cell here -- at most Mp = 1152 MFMA terms
plus a few thousand row terms, 6e-13 -- and six orders below the ~ A / (N M) one wrong element contributes (test_pass2_reference.py shows
the comparison failing on one missing (n, m) term, one missing dimension of one row and a missing kappabar N).

Inputs (seeded): X, y, bbar ~ N(0, 1), ls = 0.7 + U sqrt(d), sf2 = 1.7, kappabar = -0.7, Phibar a NON-symmetric N(0, 1) matrix (the
library symmetrises it), Z random ("rand") or M rows of X ("rows": r2 = 0 occurs, the Matern derivatives at r = 0).  Every output buffer
is filled with NaN before the call.  The comparison functions take the engine as an argument: test_pass2_reference.py runs them on the
CPU with the oracle engine.

(a) sgp_suffstats_bwd, every cell with want_gz off and on -- kbar_contract_kernel<DP, KID, GZ, KP = true>:

      N     M    d  kernel     Z      DP  what it reaches
      1     1    1  rbf        rows    2  one row, one column
      127   127  2  matern32   rows    2  one short of the tile in both directions
      128   128  3  matern52   rand    4  exactly one tile
      129   129  4  rbf        rows    4  one past the tile: two column blocks
      255   130  5  matern32   rand    8
      257   257  8  matern52   rows    8  three column blocks, two 256-row assembly blocks
      1000  129  9  rbf        rand   16  the two-pass epilogue
      1000  129  9  matern32   rows   16  the one-pass epilogue at one workgroup per CU
      700   200  16 matern52   rand   16
      333   64   17 rbf        rows   24
      333   64   18 matern32   rand   24
      500   140  24 matern52   rows   24
      300   140  25 rbf        rand   32
      300   140  32 matern32   rows   32
      300   140  32 matern52   rand   32
      2500  40   32 rbf        rows   32
      4097  257  8  rbf        rand    8  one row past 16 assembly blocks
      300   1025 3  rbf        rand    4  Mp = 1152: nine column blocks
      1     129  2  matern52   rand    2  (added: DP = 2 x matern52)
      260   131  4  matern32   rows    4  (added: DP = 4 x matern32)

    so that every (DP in 2, 4, 8, 16, 24, 32) x kernel pair occurs.  N = 0: every output exactly 0.  The cells with d in {3, 9, 32} once
    more with a caller-owned K'_fu from suffstats(..., kfu=): bit-equal.  Super-chunks (K'_fu budget = 1024 rows of the padded block:
    4 1/2 super-chunks, accumulate = 1) at (4500, 140, 3, rbf), (4500, 140, 18, rbf), (4500, 140, 5, matern52), against the reference.
(b) three of the cells, and the K_uu gradient, again with the engine's cached "bwd" / "bwd_kfu" / "kuu_bwd" workspace filled with 0xFF
    bytes (every double a NaN): bit-equal.  carve_bwd's blocks are all doubles the call writes before it reads them (scaled rows, padded
    Phibar / bbar, K'_fu, the per-workgroup sums -- read only behind the first row block that wrote them -- and the per-split partials,
    which every workgroup of the grid writes, the ones with an empty row range as zeros); sgp_kuu_bwd's two blocks likewise.  No other
    workspace is touched: the factorization and single-launch workspaces hold flag words that spinning kernels wait on.
(c) sgp_suffstats_bwd_factored(_ex) -- KP = false: kernels x d in {3, 9, 18, 32} x (N, M) in {(777, 130), (1000, 257)}, want_gz off and
    on, with and without T handed over from suffstats_whitened_rows(..., t_out=).  Phibar of the reference = L^-T (Cw / 2 s2) L^-1 in long
    double from the L^-1 read back from the device.
(d) sgp_kuu_bwd: M in {1, 2, 255, 256, 257, 1025} x d in {1, 8, 18, 32} x kernels, and (4096, 2, matern32); the per-row kernel (with g_Z)
    and the totals-only kernel (without).  The call ADDS: the buffer is pre-filled with N(0, 1) values and
    |got - (prefill + ref)| <= TAU A + 2^-52 |prefill|.
(e) SGP_KBAR_NSPLIT / SGP_KBAR_TAPER in child processes (read once per process): (4097, 257, 8, rbf) under NSPLIT = 8 (ragged shares of
    several row blocks), (32769, 64, 2, rbf) under NSPLIT = 32 with TAPER = 1 (258 blocks: the tapered map) and 0.

Largest err / A measured on an MI355X, per family (none may exceed 1e-12; anything above 1e-13 would be a finding to explain):
    (a) sgp_suffstats_bwd, 20 cells x want_gz         3.1e-16  at (333, 64, 18, matern32), want_gz on
        caller-owned K'_fu                            2.1e-16  (and bit-equal to the library-owned run)
        super-chunks                                  1.0e-16  at (4500, 140, 5, matern52)
    (c) sgp_suffstats_bwd_factored(_ex), 96 runs      9.0e-16  at (777, 130, 32, rbf), want_gz on, T recomputed
    (d) sgp_kuu_bwd, 73 cells x both kernels          5.2e-16  at (255, 32, rbf), with g_Z
    (e) knobs and splits                              2.2e-16  at (32769, 64, 2, rbf), NSPLIT = 32, TAPER = 0
"""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pass2_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SF2, KAPPABAR, S2, JITTER = 1.7, -0.7, 0.05, 1e-6
NAN = float("nan")
KERNELS = ("rbf", "matern32", "matern52")

# (N, M, d, kernel, Z from the rows of X)
CELLS = [(1, 1, 1, "rbf", True), (127, 127, 2, "matern32", True), (128, 128, 3, "matern52", False), (129, 129, 4, "rbf", True),
         (255, 130, 5, "matern32", False), (257, 257, 8, "matern52", True), (1000, 129, 9, "rbf", False),
         (1000, 129, 9, "matern32", True), (700, 200, 16, "matern52", False), (333, 64, 17, "rbf", True),
         (333, 64, 18, "matern32", False), (500, 140, 24, "matern52", True), (300, 140, 25, "rbf", False),
         (300, 140, 32, "matern32", True), (300, 140, 32, "matern52", False), (2500, 40, 32, "rbf", True),
         (4097, 257, 8, "rbf", False), (300, 1025, 3, "rbf", False), (1, 129, 2, "matern52", False), (260, 131, 4, "matern32", True)]
KFU_CELLS = [c for c in CELLS if c[2] in (3, 9, 32)]
SUPER_CELLS = [(4500, 140, 3, "rbf", False), (4500, 140, 18, "rbf", True), (4500, 140, 5, "matern52", True)]
POISON_CELLS = [(257, 257, 8, "matern52", True), (1000, 129, 9, "rbf", False), (300, 140, 32, "matern32", True)]
FACTORED_CELLS = [(N, M, d, k) for k in KERNELS for d in (3, 9, 18, 32) for (N, M) in ((777, 130), (1000, 257))]
KUU_CELLS = [(M, d, k) for k in KERNELS for M in (1, 2, 255, 256, 257, 1025) for d in (1, 8, 18, 32)] + [(4096, 2, "matern32")]
KNOB_CELLS = {"nsplit8": ((4097, 257, 8, "rbf", False), {"SGP_KBAR_NSPLIT": "8"}),
              "nsplit32_taper1": ((32769, 64, 2, "rbf", False), {"SGP_KBAR_NSPLIT": "32", "SGP_KBAR_TAPER": "1"}),
              "nsplit32_taper0": ((32769, 64, 2, "rbf", False), {"SGP_KBAR_NSPLIT": "32", "SGP_KBAR_TAPER": "0"})}


def cell_id(c):
    return "-".join(str(v) for v in c[:4]) + ("-rows" if len(c) > 4 and c[4] else "")


def test_every_dp_kernel_pair_has_a_cell():
    """The table of (a) reaches every instance kbar_contract_kernel<DP, KID, ., true> (each cell runs with GZ off and on)."""
    dp = lambda d: next(o for o in (2, 4, 8, 16, 24, 32) if d <= o)
    assert {(dp(c[2]), c[3]) for c in CELLS} == {(o, k) for o in (2, 4, 8, 16, 24, 32) for k in KERNELS}
    assert all(c[0] * c[1] * c[2] <= 10 ** 7 for c in CELLS)
    assert {(dp(c[2]), c[3]) for c in FACTORED_CELLS} == {(o, k) for o in (4, 16, 24, 32) for k in KERNELS}


# ------------------------------------------------------------------------------------------------------------------------
# inputs and references: made once per cell, shared by the tests that need them, never modified
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(N, M, d, kernel, z_rows):
    """(X, y, Z, ls, Phibar, bbar) on the CPU."""
    g = torch.Generator().manual_seed(1000003 * R.KID[kernel] + 7919 * N + 31 * M + d)
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone() if z_rows else torch.randn(M, d, dtype=torch.float64, generator=g)
    assert Z.shape[0] == M
    ls = 0.7 + torch.rand(d, dtype=torch.float64, generator=g) * math.sqrt(d)
    Pb = torch.randn(M, M, dtype=torch.float64, generator=g)
    bb = torch.randn(M, dtype=torch.float64, generator=g)
    return X, y, Z, ls, Pb, bb


@functools.lru_cache(maxsize=None)
def bwd_ref(cell):
    X, y, Z, ls, Pb, bb = inputs(*cell)
    return R.bwd_reference(X, y, Z, ls, SF2, Pb, bb, KAPPABAR, cell[3])


def on(eng, *ts):
    return [t.to(eng.device).contiguous() for t in ts]


def nan_out(eng, n):
    out = eng.empty(n)
    out.fill_(NAN)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the comparison functions (engine as an argument: HipEngine here, the oracle engine in test_pass2_reference.py)
# ------------------------------------------------------------------------------------------------------------------------
def run_bwd(eng, cell, want_gz, kfu=None):
    """suffstats_bwd on the cell's inputs into a NaN-filled buffer; the packed gradients as a CPU tensor."""
    N, M, d, kernel = cell[:4]
    X, y, Z, ls, Pb, bb = inputs(*cell)
    Xd, yd, Zd, Pd, bd = on(eng, X, y, Z, Pb, bb)
    out = nan_out(eng, d + 1 + (M * d if want_gz else 0))
    got = eng.suffstats_bwd(Xd, yd, Zd, ls.tolist(), SF2, Pd, bd, KAPPABAR, kernel, want_gz=want_gz, out=out, kfu=kfu)
    return got.cpu().clone()


def check_bwd(eng, cell, want_gz, kfu=None, what="bwd"):
    got = run_bwd(eng, cell, want_gz, kfu)
    g, A = bwd_ref(cell)
    w = R.worst_ratio(got, R.pack(g, want_gz), R.pack(A, want_gz))
    print("%s %s gz=%d: worst err/A = %.3e" % (what, cell_id(cell), want_gz, w))
    assert w <= R.TAU, (what, cell, want_gz, w)
    return got, w


def linv_square(linv, M):
    """The M x M factor inverse out of what an engine's kuu_factor returned (the HIP engine: padded to a multiple of 128, flat)."""
    flat = linv.reshape(-1)
    Mp = M if flat.numel() == M * M else (M + 127) // 128 * 128
    return flat[: Mp * Mp].reshape(Mp, Mp)[:M, :M]


def check_factored(eng, fcell):
    """suffstats_bwd_factored at one cell: want_gz off / on x T recomputed / handed over from suffstats_whitened_rows; one reference."""
    N, M, d, kernel = fcell
    X, y, Z, ls, Pb, bb = inputs(N, M, d, kernel, False)
    Cw = Pb + Pb.T
    Xd, yd, Zd, Cd, bd = on(eng, X, y, Z, Cw, bb)
    lsl = ls.tolist()
    Kuu = eng.kuu(Zd, lsl, SF2, JITTER, kernel)
    linv, info = eng.kuu_factor(Kuu)
    assert int(info.cpu()[0]) == 0
    g, A = R.bwd_factored_reference(X, y, Z, ls, SF2, linv_square(linv, M).cpu(), Cw, S2, bb, KAPPABAR, kernel)
    t = eng.kfu_buffer(N, M)
    t.fill_(NAN)
    eng.suffstats_whitened_rows(Xd, yd, Zd, lsl, SF2, linv, kernel, t_out=t)
    worst = 0.0
    for want_gz in (False, True):
        for t_in in (None, t):
            out = nan_out(eng, d + 1 + (M * d if want_gz else 0))
            got = eng.suffstats_bwd_factored(Xd, yd, Zd, lsl, SF2, linv, Cd, S2, bd, KAPPABAR, kernel, want_gz=want_gz, out=out,
                                             t_in=t_in).cpu()
            w = R.worst_ratio(got, R.pack(g, want_gz), R.pack(A, want_gz))
            print("factored %s gz=%d t_in=%d: worst err/A = %.3e" % (cell_id(fcell), want_gz, t_in is not None, w))
            assert w <= R.TAU, (fcell, want_gz, t_in is not None, w)
            worst = max(worst, w)
    return worst


@functools.lru_cache(maxsize=None)
def kuu_inputs(M, d, kernel):
    g = torch.Generator().manual_seed(77 + 1000003 * R.KID[kernel] + 31 * M + d)
    Z = torch.randn(M, d, dtype=torch.float64, generator=g)
    if M >= 2 and d in (8, 32):
        Z[M - 1] = Z[0]                                                # r2 = 0 off the diagonal as well
    ls = 0.7 + torch.rand(d, dtype=torch.float64, generator=g) * math.sqrt(d)
    Kb = torch.randn(M, M, dtype=torch.float64, generator=g)
    pre = torch.randn(d + 1 + M * d, dtype=torch.float64, generator=g)
    return Z, ls, Kb + Kb.T, pre


def run_kuu(eng, kcell, want_gz):
    M, d, kernel = kcell
    Z, ls, Kb, pre = kuu_inputs(*kcell)
    Zd, Kd = on(eng, Z, Kb)
    grads = pre.clone().to(eng.device)
    return eng.kuu_bwd(Zd, ls.tolist(), SF2, Kd, grads, kernel, want_gz=want_gz).cpu().clone()


def check_kuu(eng, kcell):
    """kuu_bwd ADDS into [g_ls | g_sf2 | g_Z]: with g_Z (the per-row kernel) and without (the totals kernel: g_Z is not touched)."""
    M, d, kernel = kcell
    Z, ls, Kb, pre = kuu_inputs(*kcell)
    g, A = R.kuu_bwd_reference(Z, ls, SF2, Kb, kernel)
    worst = 0.0
    for want_gz in (True, False):
        got = run_kuu(eng, kcell, want_gz)
        n = d + 1 + (M * d if want_gz else 0)
        assert torch.equal(got[n:], pre[n:]), "kuu_bwd without g_Z wrote behind g_sf2"
        prel = pre[:n].numpy().astype(R.LD)
        w = R.worst_ratio(got[:n], prel + R.pack(g, want_gz), R.pack(A, want_gz), slack=np.abs(prel) * R.LD(2.0) ** -52)
        print("kuu_bwd %d-%d-%s gz=%d: worst err/A = %.3e" % (kcell + (want_gz, w)))
        assert w <= R.TAU, (kcell, want_gz, w)
        worst = max(worst, w)
    return worst


# ------------------------------------------------------------------------------------------------------------------------
# (a) sgp_suffstats_bwd
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("want_gz", [False, True])
@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_pass2_against_long_double(engine, cell, want_gz):
    """Measured on an MI355X: worst err / A = 3.1e-16 over the 40 runs, at (333, 64, 18, matern32) with want_gz on."""
    check_bwd(engine, cell, want_gz)


@pytest.mark.gpu
@pytest.mark.parametrize("want_gz", [False, True])
@pytest.mark.parametrize("M,d,kernel", [(1, 1, "rbf"), (129, 9, "rbf"), (130, 9, "matern32"), (40, 32, "matern52")])
def test_pass2_empty_shard_is_exactly_zero(engine, M, d, kernel, want_gz):
    got = run_bwd(engine, (0, M, d, kernel, False), want_gz)
    assert got.numel() == d + 1 + (M * d if want_gz else 0) and bool((got == 0.0).all()), got


@pytest.mark.gpu
@pytest.mark.parametrize("cell", KFU_CELLS, ids=cell_id)
def test_pass2_caller_owned_kfu_is_bit_equal(engine, cell):
    """K'_fu kept by suffstats(..., kfu=) and handed to pass 2 against the block pass 2 assembles itself: the same bits."""
    N, M, d, kernel = cell[:4]
    X, y, Z, ls, _, _ = inputs(*cell)
    Xd, yd, Zd = on(engine, X, y, Z)
    kfu = engine.kfu_buffer(N, M)
    kfu.fill_(NAN)
    engine.suffstats(Xd, yd, Zd, ls.tolist(), SF2, kernel, kfu=kfu)
    for want_gz in (False, True):
        own, _ = check_bwd(engine, cell, want_gz, kfu=kfu, what="bwd kfu=")
        lib, _ = check_bwd(engine, cell, want_gz)
        assert torch.equal(own, lib)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", SUPER_CELLS, ids=cell_id)
def test_pass2_super_chunks_against_long_double(engine, cell):
    """accumulate = 1: 4 1/2 super-chunks of 1024 rows, the last one short, its trailing splits empty -- against the reference, not
    against pass 2.  Measured on an MI355X: worst err / A = 1.0e-16, at (4500, 140, 5, matern52) with want_gz on."""
    Mp = (cell[1] + 127) // 128 * 128
    try:
        engine.lib.sgp_set_kfu_budget_bytes(1024 * Mp * 8)
        for want_gz in (False, True):
            check_bwd(engine, cell, want_gz, what="bwd super-chunks")
    finally:
        engine.lib.sgp_set_kfu_budget_bytes(0)


# ------------------------------------------------------------------------------------------------------------------------
# (b) poisoned scratch
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cell", POISON_CELLS, ids=cell_id)
def test_pass2_does_not_read_its_scratch_before_writing_it(engine, cell):
    N, M, d, kernel = cell[:4]
    X, y, Z, ls, _, _ = inputs(*cell)
    Xd, yd, Zd = on(engine, X, y, Z)
    kfu = engine.kfu_buffer(N, M)
    engine.suffstats(Xd, yd, Zd, ls.tolist(), SF2, kernel, kfu=kfu)
    for want_gz in (False, True):
        for name, k in (("bwd", None), ("bwd_kfu", kfu)):
            first, _ = check_bwd(engine, cell, want_gz, kfu=k)
            engine._ws[name].fill_(0xFF)
            again = run_bwd(engine, cell, want_gz, kfu=k)
            assert torch.equal(first, again), (name, want_gz)


@pytest.mark.gpu
@pytest.mark.parametrize("kcell", [(257, 8, "matern52"), (130, 18, "rbf")], ids=lambda c: "%d-%d-%s" % c)
def test_kuu_bwd_does_not_read_its_scratch_before_writing_it(engine, kcell):
    for want_gz in (True, False):
        first = run_kuu(engine, kcell, want_gz)
        engine._ws["kuu_bwd"].fill_(0xFF)
        assert torch.equal(first, run_kuu(engine, kcell, want_gz)), want_gz


# ------------------------------------------------------------------------------------------------------------------------
# (c) the factored mode, (d) the K_uu gradient
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fcell", FACTORED_CELLS, ids=cell_id)
def test_pass2_factored_against_long_double(engine, fcell):
    """Measured on an MI355X: worst err / A = 9.0e-16 over the 96 runs, at (777, 130, 32, rbf), want_gz on, T recomputed (three chained
    products of up to Mp = 384 terms each stand behind every element here)."""
    check_factored(engine, fcell)


@pytest.mark.gpu
@pytest.mark.parametrize("kcell", KUU_CELLS, ids=lambda c: "%d-%d-%s" % c)
def test_pass2_kuu_bwd_against_long_double(engine, kcell):
    """Measured on an MI355X: worst err / A = 5.2e-16 over the 146 runs, at (255, 32, rbf) with g_Z."""
    check_kuu(engine, kcell)


# ------------------------------------------------------------------------------------------------------------------------
# (e) knobs and splits: read once per process, so one child process per setting
# ------------------------------------------------------------------------------------------------------------------------
CHILD = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
         "import ggp_amd, test_pass2_kernel as T\n"
         "cell, _ = T.KNOB_CELLS[sys.argv[1]]\n"
         "print(json.dumps(T.run_bwd(ggp_amd.HipEngine(), cell, True).tolist()))\n" % (ROOT, os.path.join(ROOT, "tests")))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(KNOB_CELLS))
def test_pass2_knobs_and_splits_against_long_double(engine, name):
    """The child prints the packed gradients as JSON, the parent holds them against the reference.  Measured on an MI355X: worst
    err / A = 2.2e-16, at (32769, 64, 2, rbf) under SGP_KBAR_NSPLIT = 32, SGP_KBAR_TAPER = 0."""
    cell, knobs = KNOB_CELLS[name]
    r = subprocess.run([sys.executable, "-c", CHILD, name], env=dict(os.environ, **knobs), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, r.stdout[-500:], r.stderr[-1500:])
    got = np.array(json.loads(r.stdout.strip().splitlines()[-1]), dtype=np.float64)
    g, A = bwd_ref(cell)
    w = R.worst_ratio(got, R.pack(g, True), R.pack(A, True))
    print("bwd knobs %s %s: worst err/A = %.3e" % (name, cell_id(cell), w))
    assert w <= R.TAU, (name, w)
