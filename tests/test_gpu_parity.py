"""Parity of the HIP path (through the C ABI) against the CPU oracle and the committed golden vectors.

Tolerances (fp64): statistics Phi/b are sums of products of exp() values -> 1e-12 relative to the
largest entry; the bound F -> 1e-9 * max(1,|F|) (north_star asks 1e-8 on F/N); gradients -> the
tolerance each fixture was validated at (1e-6 relative, looser for the ill-conditioned duplicate-Z
case) ; predictive mean/variance -> 1e-8 absolute.
"""
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from conftest import dev, golden_names, load_golden

pytestmark = pytest.mark.gpu

KNAME = {0: "rbf", 1: "matern32", 2: "matern52"}


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def unpack(packed, M):
    p = packed.cpu().numpy()
    return p[: M * M].reshape(M, M), p[M * M: M * M + M], p[M * M + M], p[M * M + M + 1]


# ---------------------------------------------------------------------------------------------
# dense back end
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 8, 64, 100, 128, 130, 300, 520, 1024, 2050])
def test_chol_trsm_logdiag(engine, M):
    g = torch.Generator().manual_seed(M)
    R = torch.randn(M, M + 3, dtype=torch.float64, generator=g)
    A = R @ R.T / M + torch.eye(M, dtype=torch.float64)
    L_ref = torch.linalg.cholesky(A)
    L, info = engine.chol_lower(A.to(engine.device))
    assert int(info.item()) == 0
    L = L.cpu()
    assert relerr(torch.tril(L), L_ref) < 1e-12
    B = torch.randn(M, 5, dtype=torch.float64, generator=g)
    for trans in (False, True):
        X = engine.trsm_lower(L_ref.to(engine.device).contiguous(), B.to(engine.device), trans=trans).cpu()
        X_ref = torch.linalg.solve_triangular(L_ref.T if trans else L_ref, B, upper=trans)
        assert relerr(X, X_ref) < 1e-10, (M, trans)
    ld = engine.logdiag_sum(L_ref.to(engine.device).contiguous()).item()
    assert abs(ld - torch.log(torch.diagonal(L_ref)).sum().item()) < 1e-10 * max(1, M)


def test_chain_cholesky_is_the_same_factor_for_any_number_of_workgroups(engine):
    """Round 5's single-launch factorization (csrc/sgp_potrf_chain.hpp): one chain workgroup + as many others as the CU budget leaves.
    Every work item does its arithmetic in a fixed order, so the factor must not depend on how many workgroups share the items --
    2 (one helper: a single list of items), 8 (still one list), 9 and 17 (the critical items get their own workgroups), the whole chip --
    and it must agree with LAPACK; the tile-dataflow kernel of round 1 (SGP_POTRF_CHAIN=0 in a child process) is the second opinion.
    Sizes from two block columns (no fused items at all) to thirty-two."""
    import ggp_amd
    for M in (128, 192, 320, 512, 1024, 2048):
        g = torch.Generator().manual_seed(M + 1)
        R = torch.randn(M, M + 3, dtype=torch.float64, generator=g)
        A = R @ R.T / M + torch.eye(M, dtype=torch.float64)
        L_ref = torch.linalg.cholesky(A)
        Ad = A.to(engine.device)
        L0, info = engine.chol_lower(Ad)
        assert int(info.item()) == 0 and relerr(torch.tril(L0).cpu(), L_ref) < 1e-12
        assert float(torch.triu(L0, 1).abs().max()) == 0.0                      # the strictly-upper part is zeroed, every tile of it
        # (3 ... 7: one list of items for two ... six workgroups, where FUSED_S once read tile (c+2, c) in place after FUSED_D had overwritten
        # it -- factors off by 3e-3, found by tools/potrf_budget_check.py in round 5; 17, 33: two / four workgroups for the critical items)
        for budget in (2, 3, 4, 5, 6, 7, 8, 9, 17, 33):
            e = ggp_amd.HipEngine(own_context=True)
            e.set_option("cu_budget", budget)   # (sgp_chol_lower takes no context: the engine binds its own to the thread around the call)
            for rep in range(3 if M >= 1024 else 1):
                Lb, info = e.chol_lower(Ad)
                assert int(info.item()) == 0 and torch.equal(Lb, L0), (M, budget, rep)
                e.set_option("shared_device", rep & 1)   # the ticketed claim and the static deal: the same bits


_CHAIN_CHILD = r"""
import hashlib, json, os, sys, time
import torch
sys.path.insert(0, %(root)r)
import ggp_amd
eng = ggp_amd.HipEngine()
out = {"sha": {}, "calls": 0, "mismatch": 0, "timeouts": 0}
mats = {}
for M in %(sizes)r:
    g = torch.Generator().manual_seed(M + 11)
    R = torch.randn(M, M + 3, dtype=torch.float64, generator=g)
    mats[M] = (R @ R.T / M + torch.eye(M, dtype=torch.float64)).to(eng.device)
first = {}
t_end = time.time() + %(seconds)f
while True:
    for M, A in mats.items():
        linv, info = eng.kuu_factor(A)
        L, info2 = eng.chol_lower(A)
        torch.cuda.synchronize()
        out["calls"] += 2
        if int(info.item()) == -7777 or int(info2.item()) == -7777:
            out["timeouts"] += 1
            continue
        if M not in first:
            first[M] = (linv.clone(), L.clone())
            h = hashlib.sha256(linv.cpu().numpy().tobytes()); h.update(L.cpu().numpy().tobytes())
            out["sha"][str(M)] = h.hexdigest()
        elif not (torch.equal(linv, first[M][0]) and torch.equal(L, first[M][1])):
            out["mismatch"] += 1
    if time.time() >= t_end:
        break
print("RESULT " + json.dumps(out))
"""


def _chain_children(n, sizes, seconds, env_extra=None):
    """n concurrent fresh processes on the one GPU, each factoring the same matrices (sgp_kuu_factor_ex + sgp_chol_lower) for `seconds`."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, **(env_extra or {}))
    code = _CHAIN_CHILD % {"root": ROOT, "sizes": tuple(sizes), "seconds": float(seconds)}
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for _ in range(n)]
    res = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-3000:]
        res.append(json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:]))
    return res


def test_chain_cholesky_modes_reproduce_the_default_launch_bit_for_bit(engine):
    """Round 6: with SGP_OPT_SHARED_DEVICE (environment: SGP_SHARED_DEVICE=1) the items of the chain-workgroup factorization are CLAIMED by
    ticket instead of dealt statically; SGP_POTRF_ACQUIRE=1 adds an agent-scope acquire behind every flag poll, SGP_POTRF_LIGHT=0 turns the
    same-XCD light hand-overs off.  An item's arithmetic does not depend on who runs it
    or on how its operands were published: every mode, in a fresh process each, must return the default launch's bits (factor without
    inverse and factor + inverse, M from three block columns -- the first fused items -- to thirty-two)."""
    sizes = (192, 320, 1000, 2048)
    ref = _chain_children(1, sizes, 0.0)[0]
    assert ref["timeouts"] == 0 and ref["mismatch"] == 0
    for M in sizes:   # ... and the default launch is LAPACK's factor
        g = torch.Generator().manual_seed(M + 11)
        R = torch.randn(M, M + 3, dtype=torch.float64, generator=g)
        A = R @ R.T / M + torch.eye(M, dtype=torch.float64)
        L, _ = engine.chol_lower(A.to(engine.device))
        assert relerr(torch.tril(L).cpu(), torch.linalg.cholesky(A)) < 1e-12
    for env in ({"SGP_SHARED_DEVICE": "1"}, {"SGP_POTRF_ACQUIRE": "1"}, {"SGP_POTRF_LIGHT": "0"}, {"SGP_POTRF_ACQUIRE": "1", "SGP_POTRF_LIGHT": "0", "SGP_SHARED_DEVICE": "1"},
                {"SGP_POTRF_CHAIN": "2"}):
        got = _chain_children(1, sizes, 1.0, env)[0]
        assert got["timeouts"] == 0 and got["mismatch"] == 0, (env, got)
        if "SGP_POTRF_CHAIN" in env:   # the chain kernel also where the product takes the round-1 kernel (no inverse, <= 4 block columns): the inverse's bits
            continue                   # are the chain kernel's either way, the plain factor is another kernel's there -- LAPACK agreement is asserted above
        assert got["sha"] == ref["sha"], (env, got["sha"], ref["sha"])


def test_two_processes_factorize_on_one_gpu_without_time_outs(engine):
    """the spin kernels used to need every workgroup of a launch resident at once -- two processes on one GPU
    (the reference's joblib workers, experiments/regression.py:219-231; two ranks sharing a device) each launching up to 256 spinning
    workgroups could starve each other into the 2^24-poll time-out.  With SGP_OPT_SHARED_DEVICE (the ticketed claim) an item is only ever held
    by a RUNNING workgroup and waits only for earlier tickets: three processes (this one idle, two hammering sgp_kuu_factor_ex / sgp_chol_lower at
    M = 1024 and 512 for 20 s) finish without a time-out, every call returning the single-process bits."""
    sizes = (1024, 512)
    ref = _chain_children(1, sizes, 0.0)[0]
    res = _chain_children(2, sizes, 20.0, {"SGP_SHARED_DEVICE": "1"})
    for r in res:
        assert r["timeouts"] == 0 and r["mismatch"] == 0 and r["sha"] == ref["sha"], (r, ref["sha"])
        assert r["calls"] >= 200, r["calls"]
    print("two processes on one GPU: %d + %d factorizations in 20 s, no time-out, reference bits" % (res[0]["calls"], res[1]["calls"]))


def test_chain_cholesky_forms_the_whole_inverse_inside_the_launch(engine):
    """sgp_kuu_factor's L^-1 (padded to a multiple of 128, identity in the padding) now comes out of the factorization's own launch
    (csrc/sgp_potrf_chain.hpp: INV items, block row i of L^-1 behind block column i of the factor) instead of tri_inverse()'s
    2 log2(M / 64) launches behind it: against LAPACK, exactly lower triangular, and the same bits however many workgroups share
    the items.  Sizes from two block columns to thirty-two, with and without padding."""
    import ggp_amd
    for M in (65, 128, 200, 512, 1000, 1024, 2048):
        g = torch.Generator().manual_seed(M + 5)
        R = torch.randn(M, M + 3, dtype=torch.float64, generator=g)
        A = R @ R.T / M + torch.eye(M, dtype=torch.float64)
        ref = torch.linalg.inv(torch.linalg.cholesky(A))
        Ad = A.to(engine.device)
        linv, info = engine.kuu_factor(Ad)
        Mp = int(round(math.sqrt(linv.numel())))
        Li = linv.view(Mp, Mp)
        assert int(info.item()) == 0 and relerr(Li[:M, :M].cpu(), ref) < 1e-11, (M, relerr(Li[:M, :M].cpu(), ref))
        assert float(torch.triu(Li, 1).abs().max()) == 0.0
        assert torch.equal(Li[M:, M:].cpu(), torch.eye(Mp - M, dtype=torch.float64)) and float(Li[M:, :M].abs().max() if Mp > M else 0.0) == 0.0
        for budget in (2, 3, 4, 5, 6, 7, 9, 17, 33, 40):
            e = ggp_amd.HipEngine(own_context=True)
            e.set_option("cu_budget", budget)
            for rep in range(3 if M >= 1000 else 1):
                lb, info = e.kuu_factor(Ad)
                assert int(info.item()) == 0 and torch.equal(lb, linv), (M, budget, rep)


def test_kuu_factor_ex_delivers_the_bits_of_kuu_inverse_trace(engine):
    """include/sgp.h: sgp_kuu_factor_ex writes into trace_out exactly what sgp_kuu_inverse_trace(Linv_out, M, trace_out) would -- from the
    factorization's own last launch (kuu_post_kernel) -- with the conditioning gate on or off, and leaves L^-1 / the status as sgp_kuu_factor does."""
    import ggp_amd
    n = engine.lib.sgp_kuu_inverse_trace_len()
    for M in (65, 100, 512, 1000):
        g = torch.Generator().manual_seed(M + 11)
        R = torch.randn(M, M + 3, dtype=torch.float64, generator=g)
        K = (R @ R.T / M + torch.eye(M, dtype=torch.float64)).to(engine.device)
        plain, info0 = engine.kuu_factor(K)
        for limit in (None, 0.0):
            e = ggp_amd.HipEngine(own_context=True)
            if limit is not None:
                e.set_option("cond_limit", limit)
            tr = torch.full((n,), float("nan"), dtype=torch.float64, device=engine.device)
            linv, info = e.kuu_factor(K, trace_out=tr)
            ref = e.kuu_inverse_trace(linv, M)
            assert int(info.item()) == 0 == int(info0.item()) and torch.equal(linv, plain)
            assert torch.equal(tr[:1 + M], ref[:1 + M]), (M, limit, float(tr[0]), float(ref[0]))
            assert abs(float(tr[0]) - float(torch.linalg.inv(K.cpu()).trace())) < 1e-10 * float(tr[0])


@pytest.mark.parametrize("M,pivot", [(256, 0), (256, 15), (256, 16), (256, 63), (256, 64), (256, 130), (1024, 1023), (1152, 700)])
def test_chol_reports_first_bad_pivot_of_any_tile_and_panel(engine, M, pivot):
    """LAPACK-style info = index of the first non-positive pivot, whichever work item / wave of the single-launch
    factorization meets it (tile (0,0), a fused sub-diagonal + diagonal item, any of the four 16-column panels)."""
    g = torch.Generator().manual_seed(M + pivot)
    R = torch.randn(M, M + 3, dtype=torch.float64, generator=g)
    A = R @ R.T / M + torch.eye(M, dtype=torch.float64)
    L_ref = torch.linalg.cholesky(A)
    # make the Schur complement at `pivot` negative: lower A[p][p] below the sum of squares of row p of the factor
    A[pivot, pivot] = float((L_ref[pivot, :pivot] ** 2).sum()) - 0.5
    _, info = engine.chol_lower(A.to(engine.device))
    assert int(info.item()) == pivot + 1


def test_chol_fuzz_against_lapack(engine):
    """Random sizes 1..1300: well-conditioned and ill-conditioned (cond 1e10) SPD matrices reconstruct to 1e-12, an
    indefinite matrix reports LAPACK's pivot index, a NaN is reported as a failure (never a hang, never info = 0)."""
    g = torch.Generator().manual_seed(123)
    for trial in range(32):
        M = int(torch.randint(1, 1300, (1,), generator=g))
        kind = trial % 4
        R = torch.randn(M, M, dtype=torch.float64, generator=g)
        A = R @ R.T / M + torch.eye(M, dtype=torch.float64)
        if kind == 1:
            Q, _ = torch.linalg.qr(R)
            A = (Q * torch.logspace(0, -10, M, dtype=torch.float64)) @ Q.T
            A = 0.5 * (A + A.T)
        elif kind >= 2:
            p = int(torch.randint(0, M, (1,), generator=g))
            A[p, p] = -abs(float(A[p, p])) if kind == 2 else float("nan")
        L, info = engine.chol_lower(A.to(engine.device))
        info = int(info.item())
        _, info_ref = torch.linalg.cholesky_ex(A)
        info_ref = int(info_ref)
        if kind <= 1:
            if info_ref == 0:
                Lc = torch.tril(L).cpu()
                assert info == 0 and float((Lc @ Lc.T - A).abs().max() / A.abs().max()) < 1e-12, (M, kind, info)
            else:
                assert info != 0, (M, kind)
        elif kind == 2:
            assert info == info_ref, (M, info, info_ref)
        else:
            assert info > 0, (M, info)


def test_bound_keeps_the_kuu_status_when_the_inverse_is_handed_over(engine):
    """sgp_bound_from_stats(kuu_linv=...) must not clear the status word sgp_kuu_factor wrote (include/sgp.h): one
    word, one host read, covers both factorizations; the first failure wins."""
    M, N, d = 96, 400, 2
    g = torch.Generator().manual_seed(3)
    X = torch.randn(N, d, dtype=torch.float64, generator=g).to(engine.device)
    y = torch.randn(N, dtype=torch.float64, generator=g).to(engine.device)
    Z = X[:M].clone()
    packed = engine.suffstats(X, y, Z, [1.0] * d, 1.0, "rbf")
    K = engine.kuu(Z, [1.0] * d, 1.0, 1e-6, "rbf")
    # healthy: result buffer shared by kuu_factor and bound, status 0, same F as the one-call path
    res = engine.result_buffer()
    linv, _ = engine.kuu_factor(K, info=res[2])
    out = engine.bound(K, packed, 0.1, N, kuu_linv=linv, result=res)
    o, info = engine.read_result(out["buf"].cpu())
    ref = engine.bound(K, packed, 0.1, N)
    o_ref, info_ref = engine.read_result(ref["buf"].cpu())
    assert info == 0 and info_ref == 0 and abs(float(o[0]) - float(o_ref[0])) < 1e-9 * abs(float(o_ref[0]))
    # broken Kuu: the status of kuu_factor (pivot 41) survives the second factorization
    Kbad = K.clone()
    Kbad[40, 40] = -1.0
    res = engine.result_buffer()
    linv, _ = engine.kuu_factor(Kbad, info=res[2])
    out = engine.bound(Kbad, packed, 0.1, N, kuu_linv=linv, result=res)
    _, info = engine.read_result(out["buf"].cpu())
    assert info == 41
    # ... also when it arrives as a separate tensor
    linv, kinfo = engine.kuu_factor(Kbad)
    out = engine.bound(Kbad, packed, 0.1, N, kuu_linv=linv, kuu_info=kinfo)
    assert engine.read_result(out["buf"].cpu())[1] == 41
    with pytest.raises(ValueError):
        engine.bound(K, packed, 0.1, N, kuu_linv=linv)


def test_chol_reports_non_pd_pivot(engine):
    A = torch.eye(200, dtype=torch.float64)
    A[150, 150] = -1.0
    _, info = engine.chol_lower(A.to(engine.device))
    assert int(info.item()) == 151


# ---------------------------------------------------------------------------------------------
# golden vectors: statistics, bound, gradients, predictive
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_suffstats_golden(engine, name):
    G = load_golden(name)
    M = G["Z"].shape[0]
    packed = engine.suffstats(dev(G["X"], engine), dev(G["y"], engine), dev(G["Z"], engine), G["ls"], float(G["sf2"]),
                              KNAME[int(G["kernel_id"])])
    Phi, b, yy, kappa = unpack(packed, M)
    assert relerr(Phi, G["Phi"]) < 1e-12
    assert relerr(b, G["b"]) < 1e-12
    assert abs(yy - float(G["yy"])) < 1e-12 * abs(float(G["yy"]))
    assert abs(kappa - float(G["kappa"])) < 1e-12 * abs(float(G["kappa"]))
    assert np.array_equal(Phi, Phi.T), "Phi must be exactly symmetric (mirrored, not recomputed)"


@pytest.mark.parametrize("form", ["streaming", "whitened"])
@pytest.mark.parametrize("name", golden_names())
def test_bound_and_grads_golden(engine, name, form):
    """Both evaluation orders against the fixtures.  The whitened (PyMC3) order holds 1e-9 on F and 1e-6 on every gradient
    also on the duplicate-inducing-row fixture (cond(Kuu) ~ 2e6); the streaming order loses eps * cond on F there
    (profiles/r02_logp_noise.json), its gradients (whitened adjoints) hold the same 1e-6."""
    import ggp_amd
    G = load_golden(name)
    kern = KNAME[int(G["kernel_id"])]
    cb = ggp_amd.CollapsedBound(dev(G["X"], engine), dev(G["y"], engine), kernel=kern, jitter=float(G["jitter"]), engine=engine,
                                form=form)
    Z = dev(G["Z"], engine)
    F, parts = cb.value(Z, G["ls"], float(G["sf2"]), float(G["s2"]))
    ill = float(G["grad_rtol"]) > 1e-6  # duplicate-Z fixture
    tolF = (1e-8 if ill and form == "streaming" else 1e-9) * max(1.0, abs(float(G["F"])))  # north_star: 1e-8
    assert abs(F - float(G["F"])) < tolF, (F, float(G["F"]))
    ptol = tolF * (100.0 if ill else 1.0)  # parts cancel to F; ill-conditioned fixture
    assert abs(parts["logmarg"] - float(G["logmarg"])) < ptol
    assert abs(parts["trace_term"] - float(G["trace_term"])) < ptol
    F2, g = cb.value_and_grad(Z, G["ls"], float(G["sf2"]), float(G["s2"]), want_gz=True)
    assert abs(F2 - float(G["F"])) < tolF
    rt, rz = 1e-6, (1e-4 if ill else 1e-6)  # (the fixtures' own grad_rtol / gz_rtol record the looser A.5-vs-autograd agreement)
    assert relerr(g["ls"].numpy(), G["g_ls"]) < rt, (g["ls"].numpy(), G["g_ls"])
    assert abs(g["sf2"] - float(G["g_sf2"])) < rt * max(1.0, abs(float(G["g_sf2"])))
    assert abs(g["s2"] - float(G["g_s2"])) < rt * max(1.0, abs(float(G["g_s2"])))
    assert relerr(g["Z"].cpu().numpy(), G["g_Z"]) < rz


@pytest.mark.parametrize("kernel", ["rbf", "composite"])
def test_whitened_stats_match_oracle_pymc3_order(engine, kernel):
    """sgp_suffstats_fwd_whitened: W = A A^T, u = A y with A = L^-1 K_uf against the oracle's solve_triangular form, on an
    ill-conditioned 1-D problem (inducing spacing 0.42 against a lengthscale of 3: cond(Kuu) ~ 1e8)."""
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(3)
    N, M = 634, 128
    X = torch.linspace(0, 52.8, N, dtype=torch.float64)[:, None]
    y = torch.sin(X[:, 0] * 2 * math.pi) * 0.3 + 0.04 * X[:, 0] + 0.05 * torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.linspace(0, N - 1, M).round().long()].clone()
    if kernel == "rbf":
        hyp, sf2 = [3.0], 1.3
        Kuu_ref = O.kuu(Z, torch.tensor(hyp, dtype=torch.float64), sf2, 1e-6)
        Kuf_ref = O.kern(Z, X, torch.tensor(hyp, dtype=torch.float64), sf2)
    else:
        from oracle import composite_oracle as CO
        hyp, sf2 = list(CO.co2_block(n_per=0.8, l_psmooth=1.3, l_pdecay=30.0, n_med=0.5, l_med=1.1, alpha=0.7, n_trend=1.5,
                                     l_trend=20.0, n_noise=0.1, l_noise=0.4)), 1.0
        blk = torch.tensor(hyp, dtype=torch.float64)
        Kuu_ref = CO.composite_k(Z, Z, blk) + 1e-6 * torch.eye(M, dtype=torch.float64)
        Kuf_ref = CO.composite_k(Z, X, blk)
    Xd, yd, Zd = X.to(engine.device), y.to(engine.device), Z.to(engine.device)
    Kuu = engine.kuu(Zd, hyp, sf2, 1e-6, kernel)
    linv, info = engine.kuu_factor(Kuu)
    packed = engine.suffstats_whitened(Xd, yd, Zd, hyp, sf2, linv, kernel)
    assert int(info.item()) == 0
    W, u, yy, kappa = unpack(packed, M)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(Kuu_ref), Kuf_ref, upper=False)
    Wr, ur = (A @ A.T).numpy(), (A @ y).numpy()
    assert np.max(np.abs(W - Wr)) < 1e-8 * np.max(np.abs(Wr)) and np.max(np.abs(u - ur)) < 1e-8 * np.max(np.abs(ur))
    assert np.array_equal(W, W.T) and abs(yy - float(y @ y)) < 1e-12 * float(y @ y)
    assert np.linalg.eigvalsh(W).min() > -1e-12 * np.max(np.abs(Wr))  # W = A A^T is PSD, so B = I + W / s2 cannot fail


@pytest.mark.parametrize("name", golden_names())
def test_predict_golden(engine, name):
    import ggp_amd
    G = load_golden(name)
    kern = KNAME[int(G["kernel_id"])]
    cb = ggp_amd.CollapsedBound(dev(G["X"], engine), dev(G["y"], engine), kernel=kern, jitter=float(G["jitter"]), engine=engine)
    mean, var, cov = cb.predict(dev(G["Xs"], engine), dev(G["Z"], engine), G["ls"], float(G["sf2"]), float(G["s2"]),
                                pred_noise=True, full_cov=True)
    assert np.max(np.abs(mean.cpu().numpy() - G["pred_mean"])) < 1e-8
    assert np.max(np.abs(var.cpu().numpy() - G["pred_var"])) < 1e-8
    assert np.max(np.abs(cov.cpu().numpy() - G["pred_cov"])) < 1e-8


@pytest.mark.parametrize("name", [n for n in golden_names() if n.startswith("rbf")])
def test_hmc_target_golden(engine, name):
    import ggp_amd
    G = load_golden(name)
    cb = ggp_amd.CollapsedBound(dev(G["X"], engine), dev(G["y"], engine), kernel="rbf", jitter=1e-6, engine=engine)
    tgt = ggp_amd.HmcTarget(cb, dev(G["Z"], engine))
    rt = float(G["grad_rtol"])
    for th, lp_ref, g_ref in zip(G["hmc_theta"], G["hmc_logp"], G["hmc_grad"]):
        lp, gr = tgt.logp_and_grad(th)
        ftol = (1e-9 if rt <= 1e-6 else 1e-7) * max(1.0, abs(lp_ref))  # duplicate-Z fixture: cond(Kuu) ~ 1e6
        assert abs(lp - lp_ref) < ftol
        assert relerr(np.array(gr), g_ref) < 10 * rt
        assert abs(tgt.logp(th) - lp_ref) < ftol


# ---------------------------------------------------------------------------------------------
# oracle on seeded inputs: ragged / edge shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,d", [(1, 1, 1), (15, 3, 2), (16, 5, 1), (17, 130, 4), (1000, 129, 5), (4097, 257, 8),
                                   (333, 64, 18), (2500, 40, 32), (700, 384, 3)])
def test_suffstats_vs_oracle_shapes(engine, N, M, d):
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(N * 7 + M)
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.randn(N, dtype=torch.float64, generator=g)
    Z = torch.randn(M, d, dtype=torch.float64, generator=g)
    ls = 0.7 + torch.rand(d, dtype=torch.float64, generator=g) * math.sqrt(d)
    st = O.suffstats(X, y, Z, ls, 1.7, 0)
    packed = engine.suffstats(X.to(engine.device), y.to(engine.device), Z.to(engine.device), ls.tolist(), 1.7, "rbf")
    Phi, b, yy, kappa = unpack(packed, M)
    assert relerr(Phi, st.Phi.numpy()) < 1e-12
    assert relerr(b, st.b.numpy()) < 1e-11
    assert abs(yy - st.yy) <= 1e-12 * abs(st.yy)
    assert abs(kappa - st.kappa) <= 1e-12 * abs(st.kappa)


def test_suffstats_empty_shard(engine):
    Z = torch.randn(10, 3, dtype=torch.float64).to(engine.device)
    X = torch.zeros(0, 3, dtype=torch.float64, device=engine.device)
    y = torch.zeros(0, dtype=torch.float64, device=engine.device)
    packed = engine.suffstats(X, y, Z, [1.0, 1.0, 1.0], 1.0, "rbf")
    assert float(packed.abs().max()) == 0.0


def test_gradients_vs_oracle_midsize(engine):
    """N, M past one tile in both directions; checks pass 2 against the oracle's two-pass restatement."""
    import ggp_amd
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(11)
    N, M, d = 3000, 200, 6
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    ls = 1.5 + torch.rand(d, dtype=torch.float64, generator=g)
    ref = O.grads_analytic(X, y, Z, ls, 1.2, 0.05, 1e-6, 0)
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), jitter=1e-6, engine=engine)
    F, gr = cb.value_and_grad(Z.to(engine.device), ls.tolist(), 1.2, 0.05, want_gz=True)
    assert abs(F - ref["F"]) < 1e-9 * abs(ref["F"])
    assert relerr(gr["ls"].numpy(), ref["g_ls"].numpy()) < 1e-6
    assert abs(gr["sf2"] - ref["g_sf2"]) < 1e-6 * abs(ref["g_sf2"])
    assert abs(gr["s2"] - ref["g_s2"]) < 1e-6 * abs(ref["g_s2"])
    assert relerr(gr["Z"].cpu().numpy(), ref["g_Z"].numpy()) < 1e-5


def test_not_pd_is_reported_not_raised_in_hmc(engine):
    import ggp_amd
    X = torch.randn(50, 2, dtype=torch.float64)
    y = torch.randn(50, dtype=torch.float64)
    Z = torch.zeros(6, 2, dtype=torch.float64)  # six identical inducing rows, no jitter -> singular Kuu
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), jitter=0.0, engine=engine)
    with pytest.raises(ggp_amd.NotPositiveDefiniteError):
        cb.value(Z.to(engine.device), [1.0, 1.0], 1.0, 0.1)
    F, parts = cb.value(Z.to(engine.device), [1.0, 1.0], 1.0, 0.1, raise_on_fail=False)
    assert math.isnan(F) and parts["info"] > 0


# ---------------------------------------------------------------------------------------------
# size-independent properties at the BASELINE C5 shape (N = 1M, M = 1024, d = 8)
# ---------------------------------------------------------------------------------------------
def _c5(engine, N=1_000_000, M=1024, d=8):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    w = torch.randn(d, dtype=torch.float64, generator=g) / math.sqrt(d)
    y = torch.sin(X @ w) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    y = (y - y.mean()) / y.std()
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    return X.to(engine.device), y.to(engine.device), Z.to(engine.device)


def test_c5_shard_additivity_and_determinism(engine):
    X, y, Z = _c5(engine)
    M = Z.shape[0]
    ls = [2.0] * 8
    full = engine.suffstats(X, y, Z, ls, 1.0, "rbf").clone()
    again = engine.suffstats(X, y, Z, ls, 1.0, "rbf").clone()
    assert torch.equal(full, again), "pass 1 must be bit-reproducible"
    parts = torch.zeros_like(full)
    for lo, hi in ((0, 333_333), (333_333, 700_001), (700_001, 1_000_000)):
        parts += engine.suffstats(X[lo:hi].contiguous(), y[lo:hi].contiguous(), Z, ls, 1.0, "rbf")
    assert float((parts - full).abs().max() / full.abs().max()) < 1e-13
    Phi = full[: M * M].reshape(M, M)
    assert torch.equal(Phi, Phi.T)
    # diag(Phi) = sum_n k(z_m, x_n)^2 <= N sf2^2 ; trace identity against a direct fp64 evaluation on a slice
    assert float(Phi.diagonal().max()) <= 1_000_000.0
    m = 7
    kcol = torch.exp(-0.5 * (((X - Z[m]) / 2.0) ** 2).sum(1))
    assert abs(float(Phi[m, m]) - float((kcol * kcol).sum())) < 1e-10 * float(Phi[m, m])
    assert abs(float(full[M * M + m]) - float((kcol * y).sum())) < 1e-9 * max(1.0, abs(float(full[M * M + m])))


def test_c5_bound_matches_chunked_oracle_on_subsample(engine):
    """Full-size shape is too slow for the oracle; N = 20k of the same data at M = 1024 finishes in seconds."""
    import ggp_amd
    from oracle import vfe_oracle as O
    X, y, Z = _c5(engine, N=20_000)
    cb = ggp_amd.CollapsedBound(X, y, jitter=1e-6, engine=engine)
    F, _ = cb.value(Z, [2.0] * 8, 1.0, 0.09)
    F_ref = O.vfe_pymc3_order_chunked(X.cpu(), y.cpu(), Z.cpu(), torch.full((8,), 2.0, dtype=torch.float64), 1.0, 0.3, 1e-6)
    assert abs(F - F_ref) < 1e-8 * abs(F_ref), (F, F_ref)


def test_streaming_without_resident_kfu_and_with_super_chunks(engine):
    """Three ways to hold K'_fu must agree bit for bit in pass 1 and to rounding in pass 2: caller-owned block,
    library-owned single block, library-owned super-chunks (budget shrunk so 5 000 rows need several)."""
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(5)
    N, M, d = 5000, 140, 3
    X = torch.randn(N, d, dtype=torch.float64, generator=g).to(engine.device)
    y = torch.randn(N, dtype=torch.float64, generator=g).to(engine.device)
    Z = torch.randn(M, d, dtype=torch.float64, generator=g).to(engine.device)
    ls = [1.1, 0.8, 1.4]
    Pb = torch.randn(M, M, dtype=torch.float64, generator=g)
    Pb = (Pb + Pb.T).to(engine.device).contiguous()
    bb = torch.randn(M, dtype=torch.float64, generator=g).to(engine.device)
    kfu = engine.kfu_buffer(N, M)
    p_own = engine.suffstats(X, y, Z, ls, 1.3, "rbf", kfu=kfu).clone()
    g_own = engine.suffstats_bwd(X, y, Z, ls, 1.3, Pb, bb, -0.7, "rbf", want_gz=True, kfu=kfu).clone()
    p_lib = engine.suffstats(X, y, Z, ls, 1.3, "rbf").clone()
    g_lib = engine.suffstats_bwd(X, y, Z, ls, 1.3, Pb, bb, -0.7, "rbf", want_gz=True).clone()
    assert torch.equal(p_own, p_lib) and torch.equal(g_own, g_lib)
    # K'_fu itself against the oracle's kernel matrix
    Kref = O.kern(X.cpu(), Z.cpu(), torch.tensor(ls, dtype=torch.float64), 1.0)
    Kdev = kfu.reshape(-1, 256)[:N, :M].cpu()
    assert float((Kdev - Kref).abs().max()) < 1e-14
    try:
        engine.lib.sgp_set_kfu_budget_bytes(1024 * 256 * 8)  # 1024 rows of a 256-column block at a time
        p_sc = engine.suffstats(X, y, Z, ls, 1.3, "rbf").clone()
        g_sc = engine.suffstats_bwd(X, y, Z, ls, 1.3, Pb, bb, -0.7, "rbf", want_gz=True).clone()
    finally:
        engine.lib.sgp_set_kfu_budget_bytes(0)
    assert float((p_sc - p_lib).abs().max() / p_lib.abs().max()) < 1e-13
    assert float((g_sc - g_lib).abs().max() / g_lib.abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------
# model classes on the device (reference call pattern: construct -> train_model -> posterior_predictive)
# ---------------------------------------------------------------------------------------------
def test_sparse_gpr_training_trace_on_device(engine):
    import ggp_amd
    from test_models_hmc import demo_1d, reference_loss_trace
    X, y, Xt, Z0 = demo_1d()
    model = ggp_amd.SparseGPR(X.to(engine.device), y.to(engine.device), ggp_amd.GaussianLikelihood(), Z0, engine=engine, jitter=1e-6)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses = model.train_model(opt, max_steps=12, verbose=False)
    ref = reference_loss_trace(X, y, Z0, 12, 0.01, jitter=1e-6)
    assert np.max(np.abs(np.array(losses[:2]) - np.array(ref[:2]))) < 1e-10
    assert np.max(np.abs(np.array(losses) - np.array(ref))) < 1e-6
    pred = model.posterior_predictive(Xt.to(engine.device))
    assert pred.loc.shape == (200,) and pred.covariance_matrix.shape == (200, 200)
    assert math.isfinite(float(ggp_amd.nlpd(pred, torch.sin(Xt * 3), torch.tensor([1.0]))))


def test_bayesian_sgpr_hmc_on_device(engine):
    import ggp_amd
    from oracle import vfe_oracle as O
    from test_models_hmc import small_problem
    X, y, Z0, Xt = small_problem()
    model = ggp_amd.BayesianSparseGPR_HMC(X.to(engine.device), y.to(engine.device), ggp_amd.GaussianLikelihood(), Z0,
                                          engine=engine, seed=7)
    trace, steps, perf = model.train_fixed_model(num_tune=40, num_samples=15)
    assert len(trace) == 15 and np.all(trace["ls"] > 0)
    th = trace[3]["theta_unc"]
    lp_ref, _ = O.hmc_logp(torch.tensor(th), X, y, Z0[:, None])
    assert abs(trace.get_sampler_stats("logp")[3] - lp_ref) < 1e-8 * max(1.0, abs(lp_ref))
    preds = ggp_amd.mixture_posterior_predictive(model, Xt.to(engine.device), trace)
    assert 1 <= len(preds) <= 15
    assert math.isfinite(ggp_amd.nlpd_mixture(preds, torch.sin(Xt), torch.tensor([1.0])))


def test_side_stream_tail_overlap_matches_serial(engine):
    """Kuu factorised on a second stream under pass 1 (default) vs everything on one stream: same numbers."""
    import ggp_amd
    G = load_golden("rbf_d18_mid")
    cb = ggp_amd.CollapsedBound(dev(G["X"], engine), dev(G["y"], engine), jitter=float(G["jitter"]), engine=engine)
    Z = dev(G["Z"], engine)
    outs = []
    for ov in (True, False, True, True):
        cb.overlap_tail, cb.overlap_min_work = ov, 0  # force the two-stream path at this small size
        F, g = cb.value_and_grad(Z, G["ls"], float(G["sf2"]), float(G["s2"]), want_gz=True)
        outs.append((F, g["ls"].clone(), g["Z"].clone()))
    assert outs[0][0] == outs[1][0] == outs[2][0] == outs[3][0]
    assert all(torch.equal(outs[0][1], o[1]) and torch.equal(outs[0][2], o[2]) for o in outs[1:])
    # a singular Kuu is still reported through the merged info flag
    Zbad = torch.zeros(6, 18, dtype=torch.float64, device=engine.device)
    cb0 = ggp_amd.CollapsedBound(dev(G["X"], engine), dev(G["y"], engine), jitter=0.0, engine=engine)
    F, parts = cb0.value(Zbad, G["ls"], 1.0, 0.1, raise_on_fail=False)
    assert math.isnan(F) and 1 <= parts["info"] <= 6


def test_evaluation_is_the_same_bits_under_any_cu_budget(engine):
    """The CU budget of a context (SGP_OPT_CU_BUDGET: a caller on a CU-masked stream) only changes how many workgroups share the work
    items of the two factorizations -- never an evaluation's bits: value and gradients at a C3-like shape (two-stream path, chain Cholesky
    with the inverse inside, M = 512) for budgets 3 ... 40 against the whole chip."""
    import ggp_amd
    g = torch.Generator().manual_seed(21)
    N, d, M = 6000, 5, 512
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    ref = None
    for budget in (0, 3, 4, 5, 7, 9, 17, 40):
        e = ggp_amd.HipEngine(own_context=True)
        if budget:
            e.set_option("cu_budget", budget)
        cb = ggp_amd.CollapsedBound(X.to(e.device), y.to(e.device), jitter=1e-6, engine=e)
        for rep in range(3):
            F, gr = cb.value_and_grad(Z.to(e.device), [1.5] * d, 1.0, 0.05, want_gz=True)
            cur = (F, gr["ls"].clone(), gr["sf2"], gr["s2"], gr["Z"].cpu().clone())
            if ref is None:
                ref = cur
            assert cur[0] == ref[0] and torch.equal(cur[1], ref[1]) and cur[2] == ref[2] and cur[3] == ref[3] and torch.equal(cur[4], ref[4]), \
                (budget, rep, cur[0], ref[0])


def test_largest_supported_inducing_set(engine):
    """M = SGP_MAX_INDUCING = 4096: 2080 tiles over 256 persistent workgroups in the dataflow Cholesky, the widest
    kernel-matrix rows, and one past the limit is refused."""
    import ggp_amd
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(9)
    N, M, d = 6000, 4096, 4
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Z = torch.randn(M, d, dtype=torch.float64, generator=g) * 1.5
    ls, sf, sn = [0.7] * d, 1.1, 0.3
    F_ref = float(O.vfe_pymc3_order(X, y, Z, ls, sf, sn, 1e-6))
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), jitter=1e-6, engine=engine)
    F, parts = cb.value(Z.to(engine.device), ls, sf * sf, sn * sn)
    assert abs(F - F_ref) < 1e-8 * abs(F_ref), (F, F_ref)
    F2, gr = cb.value_and_grad(Z.to(engine.device), ls, sf * sf, sn * sn)
    # (value-only evaluations of this much work contract on the integer matrix cores, value + gradient ones on the fp64 cores:
    # the same Phi to ~1e-15 of its largest entry, not bit for bit; with one contraction for both they are identical)
    assert abs(F2 - F) < 1e-10 * abs(F) and gr["info"] == 0 and np.all(np.isfinite(gr["ls"].numpy()))
    prev = engine.lib.sgp_set_contraction(0)
    try:
        F0, _ = cb.value(Z.to(engine.device), ls, sf * sf, sn * sn)
        F20, _ = cb.value_and_grad(Z.to(engine.device), ls, sf * sf, sn * sn)
    finally:
        engine.lib.sgp_set_contraction(prev)
    assert F20 == F0
    with pytest.raises((ggp_amd.SgpStatusError, ValueError)):
        cb.value(torch.randn(M + 1, d, dtype=torch.float64).to(engine.device), ls, sf * sf, sn * sn)


def test_integration_md_ctypes_stub_runs(engine):
    """The binding shown to a reference maintainer in INTEGRATION.md (section B) is executed verbatim."""
    import re
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", text, flags=re.S)
    stub = next(b for b in blocks if "def elbo(" in b)
    stub = stub.replace('C.CDLL("generalised-gaussian-processes_amd/csrc/libsgp_hip.so")',
                        "C.CDLL(%r)" % os.path.join(ROOT, "generalised-gaussian-processes_amd", "csrc", "libsgp_hip.so"))
    ns = {}
    exec(compile(stub, "INTEGRATION.md", "exec"), ns)
    G = load_golden("rbf_d3_small")
    F = ns["elbo"](dev(G["X"], engine), dev(G["y"], engine), dev(G["Z"], engine), G["ls"].tolist(), float(G["sf2"]), float(G["s2"]),
                   jitter=float(G["jitter"]))
    assert abs(F - float(G["F"])) < 1e-9 * max(1.0, abs(float(G["F"])))


@pytest.mark.parametrize("knob", ["SGP_SYRK_GLDS=1", "SGP_SYRK_WAVES=8", "SGP_SYRK_SKIP_UPPER=0", "SGP_TARGET_WGS=512", "SGP_SYRK_TAPER=0",
                                  "SGP_SYRK_NSPLIT=24", "SGP_KBAR_NSPLIT=40", "SGP_KBAR_TAPER=0"])
def test_tuning_knobs_do_not_change_results(engine, knob):
    """The A/B knobs of the pass-1 contraction (LDS-DMA staging, 8-wave workgroups, full diagonal tiles, fewer splits) are
    read once per process, so each runs in a child process; all must reproduce the golden sufficient statistics.  The two
    SGP_KBAR_* knobs belong to pass 2: every child also runs suffstats_bwd on the fixture with a fixed random (non-symmetric) Phibar
    and bbar, against the oracle engine's float64 restatement -- component-wise within 1e-12 of the condition scale A of
    tests/pass2_reference.py (the oracle engine itself stays within 2e-16 A of the long-double reference)."""
    import subprocess
    import sys as _sys
    code = (
        "import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ggp_amd; from conftest import load_golden, dev\n"
        "eng = ggp_amd.HipEngine(); G = load_golden('rbf_d18_mid')\n"
        "full = eng.suffstats(dev(G['X'], eng), dev(G['y'], eng), dev(G['Z'], eng), G['ls'], float(G['sf2'])).cpu().numpy()\n"
        "M = G['Z'].shape[0]; Phi = full[:M*M].reshape(M, M)\n"
        "assert np.abs(Phi - G['Phi']).max() < 1e-12 * np.abs(G['Phi']).max(), np.abs(Phi - G['Phi']).max()\n"
        "assert np.abs(full[M*M:M*M+M] - G['b']).max() < 1e-12 * np.abs(G['b']).max()\n"
        "import pass2_reference as R; from fake_engine import OracleEngine\n"
        "g = torch.Generator().manual_seed(17); Pb = torch.randn(M, M, dtype=torch.float64, generator=g)\n"
        "bb = torch.randn(M, dtype=torch.float64, generator=g)\n"
        "X, y, Z = (torch.as_tensor(np.ascontiguousarray(G[k]), dtype=torch.float64) for k in 'XyZ'); ls, sf2 = G['ls'].tolist(), float(G['sf2'])\n"
        "got = eng.suffstats_bwd(dev(X, eng), dev(y, eng), dev(Z, eng), ls, sf2, dev(Pb, eng), dev(bb, eng), -0.7, 'rbf', want_gz=True).cpu()\n"
        "ref = OracleEngine().suffstats_bwd(X, y, Z, ls, sf2, Pb, bb, -0.7, 'rbf', want_gz=True)\n"
        "A = R.pack(R.bwd_reference(X, y, Z, ls, sf2, Pb, bb, -0.7, 'rbf')[1], True)\n"
        "w = R.worst_ratio(got, ref.numpy().astype(R.LD), A); print('pass 2: worst err / A = %%.3e' %% w); assert w <= 1e-12, w\n"
        "print('ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ)
    k, v = knob.split("=")
    env[k] = v
    r = subprocess.run([_sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (knob, r.stdout[-500:], r.stderr[-1500:])


def test_tapered_splits_match_equal_splits(engine):
    """At sizes where the split counts taper (default), F and the gradients must agree with equal splits to rounding
    (only the order of the fixed-order partial sums changes).  One child process per setting: the knobs are static."""
    import json
    import subprocess
    import sys as _sys
    code = (
        "import sys, json, math, torch; sys.path.insert(0, %r)\n"
        "import ggp_amd\n"
        "eng = ggp_amd.HipEngine(); g = torch.Generator().manual_seed(4)\n"
        "N, M, d = 300000, 1024, 8\n"
        "X = torch.randn(N, d, dtype=torch.float64, generator=g); w = torch.randn(d, dtype=torch.float64, generator=g) / math.sqrt(d)\n"
        "y = torch.sin(X @ w) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)\n"
        "Z = X[torch.randperm(N, generator=g)[:M]].clone().to(eng.device)\n"
        "cb = ggp_amd.CollapsedBound(X.to(eng.device), y.to(eng.device), jitter=1e-6, engine=eng)\n"
        "F, gr = cb.value_and_grad(Z, [2.0] * d, 1.0, 0.09, want_gz=True)\n"
        "print(json.dumps({'F': F, 'ls': gr['ls'].tolist(), 'sf2': gr['sf2'], 's2': gr['s2'], 'gz': gr['Z'].cpu().flatten()[:64].tolist(),\n"
        "                  'gzn': float(gr['Z'].norm())}))\n" % ROOT)
    outs = []
    for taper in ("1", "0"):
        # (SGP_CONTRACTION=0: the tapered splits of pass 1 belong to the fp64 contraction; pass 2 tapers either way)
        env = dict(os.environ, SGP_SYRK_TAPER=taper, SGP_KBAR_TAPER=taper, SGP_CONTRACTION="0")
        r = subprocess.run([_sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    a, b = outs
    # rounding of Phi (1e-16 per entry) is amplified by cond(Kuu) ~ 1e6 at jitter 1e-6: 3e-10 relative in F was observed
    assert abs(a["F"] - b["F"]) < 1e-8 * abs(b["F"])
    for k in ("ls", "gz"):
        assert np.abs(np.array(a[k]) - np.array(b[k])).max() < 1e-6 * max(1.0, np.abs(np.array(b[k])).max())
    assert abs(a["sf2"] - b["sf2"]) < 1e-6 * abs(b["sf2"]) and abs(a["s2"] - b["s2"]) < 1e-6 * abs(b["s2"])
    assert abs(a["gzn"] - b["gzn"]) < 1e-6 * b["gzn"]


def test_repeated_evaluations_all_modes_stay_clean(engine):
    """Regression: many evaluations over several M, fresh CollapsedBound objects (new side-stream buffers and events), two streams /
    single stream.  The single-launch dataflow Cholesky must never report its
    time-out code and every mode must give the same bits (a stale flag word once showed up as info = -7777)."""
    import ggp_amd
    g = torch.Generator().manual_seed(3)
    for rep in range(3):
        for (N, d, M) in [(400, 1, 8), (2000, 18, 128), (64, 3, 30), (500, 2, 6), (1000, 5, 129)]:
            X = torch.randn(N, d, dtype=torch.float64, generator=g).to(engine.device)
            y = torch.randn(N, dtype=torch.float64, generator=g).to(engine.device)
            Z = X[:M].clone()
            cb = ggp_amd.CollapsedBound(X, y, jitter=1e-6, engine=engine)
            vals = []
            for mode in (True, True, False):
                cb.overlap_tail, cb.overlap_min_work = mode, 0  # two-stream path even when tiny
                for _ in range(4):
                    F, parts = cb.value(Z, [1.0] * d, 1.0, 0.1, raise_on_fail=False)
                    assert parts["info"] == 0, (rep, N, d, M, mode, parts)
                    F2, gr = cb.value_and_grad(Z, [1.0] * d, 1.0, 0.1, raise_on_fail=False)
                    assert gr["info"] == 0 and F2 == F
                    vals.append(F)
            assert all(v == vals[0] for v in vals)


# ---------------------------------------------------------------------------------------------
# BASELINE.json configs C1-C3 at their full sizes (synthetic stand-ins)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,d,M", [("C1_demo1d", 500, 1, 50), ("C2_co2", 634, 1, 128), ("C3_elevators", 13279, 18, 512)])
def test_baseline_configs_match_cpu_to_1e8_per_datum(engine, name, N, d, M):
    """north_star: 'ELBO matches CPU to 1e-8' -- asserted on F/N (GPyTorch's mll convention), value and gradient."""
    import ggp_amd
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(N + M)
    if d == 1:
        X = torch.linspace(0.0, 52.8, N, dtype=torch.float64)[:, None] if "co2" in name else torch.randn(N, 1, dtype=torch.float64, generator=g) * 2 - 1
        y = torch.sin(X[:, 0] * (2.0 if "co2" in name else 3.0)) + 0.05 * X[:, 0] + 0.2 * torch.randn(N, dtype=torch.float64, generator=g)
        ls = torch.tensor([1.5 if "co2" in name else 0.7], dtype=torch.float64)
    else:
        X = torch.randn(N, d, dtype=torch.float64, generator=g)
        w = torch.randn(d, dtype=torch.float64, generator=g) / math.sqrt(d)
        y = torch.sin(X @ w) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
        ls = torch.full((d,), 3.0, dtype=torch.float64)
    y = (y - y.mean()) / y.std()
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    sf2, s2 = 1.0, 0.09
    F_ref = O.vfe_pymc3_order_chunked(X, y, Z, ls, 1.0, 0.3, 1e-6)
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), jitter=1e-6, engine=engine)
    F, gr = cb.value_and_grad(Z.to(engine.device), ls.tolist(), sf2, s2, want_gz=False)
    assert abs(F - F_ref) / N < 1e-8, (name, F, F_ref)
    # gradients at the FULL size of every config (C3: 13 279 x 512, autograd through the PyMC3-order graph, ~2 s of host
    # time): 1e-6 relative -- the whitened adjoints hold it also where cond(Kuu) ~ 1 / jitter (C1 / C2: 1-D inputs)
    ref = O.grads_autograd(X, y, Z, ls, sf2, s2, 1e-6)
    assert float((gr["ls"] - ref["g_ls"]).abs().max()) < 1e-6 * max(1.0, float(ref["g_ls"].abs().max()))
    assert abs(gr["s2"] - ref["g_s2"]) < 1e-6 * max(1.0, abs(ref["g_s2"]))
    assert abs(gr["sf2"] - ref["g_sf2"]) < 1e-6 * max(1.0, abs(ref["g_sf2"]))
    Fz, gz = cb.value_and_grad(Z.to(engine.device), ls.tolist(), sf2, s2, want_gz=True)
    assert relerr(gz["Z"].cpu().numpy(), ref["g_Z"].numpy()) < 1e-5


def test_c5_full_size_value_on_all_rows_and_gradients_on_100k(engine):
    """The headline configuration itself (N = 1 000 000, d = 8, M = 1024): F on ALL rows against the chunked CPU oracle
    (north_star: 1e-8; ~80-110 s of host time), and the leapfrog's gradients at M = 1024 on the first 100 000 rows against
    torch autograd through the PyMC3-order graph (~35 s)."""
    import bench
    import ggp_amd
    from oracle import vfe_oracle as O
    N, M, d = bench.N_TOTAL, bench.M_IND, bench.DIM
    X, y, Z = bench.synth(N, M, d)
    cb = ggp_amd.CollapsedBound(X.to(engine.device), y.to(engine.device), jitter=bench.JITTER, engine=engine)
    F_hip, parts = cb.value(Z.to(engine.device), [bench.LS] * d, bench.SF ** 2, bench.SN ** 2)
    del cb
    torch.set_num_threads(os.cpu_count() or 1)
    F_cpu = O.vfe_pymc3_order_chunked(X, y, Z, [bench.LS] * d, bench.SF, bench.SN, bench.JITTER)
    assert abs(F_hip - F_cpu) < 1e-8 * abs(F_cpu), (F_hip, F_cpu)
    GR = 100_000
    Xg, yg = X[:GR], y[:GR]
    cbg = ggp_amd.CollapsedBound(Xg.to(engine.device), yg.to(engine.device), jitter=bench.JITTER, engine=engine)
    Fg, g = cbg.value_and_grad(Z.to(engine.device), [bench.LS] * d, bench.SF ** 2, bench.SN ** 2, want_gz=True)
    ref = O.grads_autograd(Xg, yg, Z, [bench.LS] * d, bench.SF ** 2, bench.SN ** 2, bench.JITTER)
    assert abs(Fg - ref["F"]) < 1e-8 * abs(ref["F"])
    assert relerr(g["ls"].numpy(), ref["g_ls"].numpy()) < 1e-6
    assert abs(g["sf2"] - ref["g_sf2"]) < 1e-6 * abs(ref["g_sf2"]) and abs(g["s2"] - ref["g_s2"]) < 1e-6 * abs(ref["g_s2"])
    assert relerr(g["Z"].cpu().numpy(), ref["g_Z"].numpy()) < 1e-5


@pytest.mark.parametrize("fused", [True, False])
def test_bayesian_sgpr_hmc_alternating_schedule_on_device(engine, fused):
    """Row a7 on the HIP path (reference models/bayesian_sgpr_hmc.py:100-157): warm-start Adam steps, then NUTS at the
    scheduled iterations with the kernel hyper-parameters frozen and the loss averaged over the current theta samples,
    back-propagated to Z only.  Same seeds on the device and on the CPU test double: the loss traces must agree (the
    samplers see log-densities that differ at 1e-10, so the chains -- hence the averaged losses -- coincide to ~1e-6).
    Both the single-launch (device-resident sampler) and the multi-launch path."""
    import ggp_amd
    from fake_engine import OracleEngine
    from test_models_hmc import small_problem
    X, y, Z0, Xt = small_problem()
    kw = dict(max_steps=9, hmc_scheduler=[3, 6, 8], verbose=False, num_tune_long=15, num_samples_long=4, num_tune_short=8,
              num_samples_short=3)
    out = []
    for eng in (engine, OracleEngine()):
        Xd, yd = (X.to(eng.device), y.to(eng.device))
        model = ggp_amd.BayesianSparseGPR_HMC(Xd, yd, ggp_amd.GaussianLikelihood(), Z0, engine=eng, seed=11, jitter=1e-6)
        model.device_sampler = False  # both runs through hmc.NUTS with numpy's generator: comparable draw for draw
        if eng is engine:
            model._bound().fused = fused
            model._hmc_bound().fused = fused
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        losses, trace, step_sizes, perf = model.train_model(opt, **kw)
        out.append((losses, trace, model.inducing_points.detach().cpu().clone(),
                    [n for n, p in model.named_parameters() if not p.requires_grad]))
    (la, ta, za, fa), (lb, tb, zb, fb) = out
    assert len(la) == len(lb) == 3 + 5 and len(ta) == len(tb) == 4
    assert np.max(np.abs(np.array(la) - np.array(lb))) < 1e-6 * max(1.0, np.max(np.abs(lb))), (la, lb)
    assert np.allclose(ta["ls"], tb["ls"], rtol=1e-5) and np.allclose(ta["sig_n"], tb["sig_n"], rtol=1e-5)
    assert float((za - zb).abs().max()) < 1e-6
    assert fa == fb and 'covar_module.inducing_points' not in fa and len(fa) == 3
    # and with the device-resident sampler the schedule runs end to end
    model = ggp_amd.BayesianSparseGPR_HMC(X.to(engine.device), y.to(engine.device), ggp_amd.GaussianLikelihood(), Z0, engine=engine,
                                          seed=11, jitter=1e-6)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    losses, trace, step_sizes, perf = model.train_model(opt, **kw)
    assert len(losses) == 8 and all(math.isfinite(v) for v in losses) and len(trace) == 4
    assert getattr(trace, "device_resident", False) and len(step_sizes) == 3 and all(p > 0 for p in perf)


def test_mixture_predictive_stays_on_the_device(engine, monkeypatch):
    """Row f-2 (reference models/bayesian_sgpr_hmc.py:198-231, utils/metrics.py:42-67): per-sample predictives with the PSD
    gate cholesky(cov + 1e-4 I) and the joint nlpd -- T x T covariances are factored on the GPU (sgp_chol_lower /
    sgp_trsm_lower / sgp_logdiag_sum); nothing larger than a T-vector crosses PCIe.  nlpd_mixture against the oracle."""
    import ggp_amd
    from oracle import vfe_oracle as O
    from ggp_amd.hmc import Trace
    g = torch.Generator().manual_seed(5)
    N, M, T, d = 1500, 60, 700, 2
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X[:, 0]) * torch.cos(X[:, 1]) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Xt = torch.randn(T, d, dtype=torch.float64, generator=g)
    yt = torch.sin(Xt[:, 0]) * torch.cos(Xt[:, 1]) + 0.1 * torch.randn(T, dtype=torch.float64, generator=g)
    Z0 = X[torch.randperm(N, generator=g)[:M]].clone()
    model = ggp_amd.BayesianSparseGPR_HMC(X.to(engine.device), y.to(engine.device), ggp_amd.GaussianLikelihood(), Z0, engine=engine,
                                          jitter=1e-6)
    rows = [{"ls": np.array([0.9 + 0.1 * i, 1.2 - 0.05 * i]), "sig_f": 1.0 + 0.05 * i, "sig_n": 0.3 + 0.02 * i} for i in range(5)]
    trace = Trace(rows, {"step_size": np.zeros(5)})
    moved = []
    real_to = torch.Tensor.to

    def spy_to(self, *a, **k):
        tgt = a[0] if a else k.get("device")
        if self.is_cuda and (tgt == "cpu" or (isinstance(tgt, torch.device) and tgt.type == "cpu")):
            moved.append(self.numel())
        return real_to(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "to", spy_to)
    preds = ggp_amd.mixture_posterior_predictive(model, Xt.to(engine.device), trace)
    val = ggp_amd.nlpd_mixture(preds, yt, torch.tensor([1.0]))
    monkeypatch.undo()
    assert len(preds) == 5 and all(p.covariance_matrix.is_cuda for p in preds)
    assert max(moved, default=0) <= T, "a T x T matrix was copied to the host: %r" % (sorted(set(moved))[-3:],)
    ref = []
    for r in rows:
        mu, cov = O.predict(Xt, X, y, Z0, torch.as_tensor(r["ls"]), r["sig_f"] ** 2, r["sig_n"] ** 2, 1e-6, full_cov=True)
        ref.append(O.nlpd_joint(mu, cov, yt, 1.0))
    assert abs(val - float(np.mean(ref))) < 1e-7 * max(1.0, abs(float(np.mean(ref)))), (val, float(np.mean(ref)))


def test_kernel_exp_accuracy(engine):
    """The hand-rolled exp() of the kernel profiles (csrc/sgp_common.hpp: sgp_exp) against libm over its whole range: the first
    row of a 1-D RBF Kuu with unit lengthscale is exp(-z_i^2 / 2).  <= 2.5e-16 relative (1-2 ulp), exact 1 at 0, clean underflow."""
    t = np.concatenate([np.linspace(0.0, 40.0, 2000), np.linspace(40.0, 744.0, 2000), [745.2, 760.0, 1.0e4]])
    z = np.concatenate([[0.0], np.sqrt(2.0 * t)])
    M = z.size
    K = engine.kuu(dev(z[:, None], engine), [1.0], 1.0, 0.0, "rbf").cpu().numpy()
    ref = np.exp(-0.5 * (z * z))
    got = K[0]
    assert got[0] == 1.0 and got[1] == 1.0
    big = ref > 1e-300
    assert np.max(np.abs(got[big] - ref[big]) / ref[big]) < 2.5e-16, np.max(np.abs(got[big] - ref[big]) / ref[big])
    assert np.all(np.abs(got[~big] - ref[~big]) <= 1e-300) and np.all(np.isfinite(got)) and np.all(got >= 0.0)
    # a NaN input must come out as NaN (a clamp by fmax() would turn a corrupt distance into k = 0 and a finite, meaningless bound)
    zn = np.array([[0.0], [1.0], [np.nan]])
    Kn = engine.kuu(dev(zn, engine), [1.0], 1.0, 0.0, "rbf").cpu().numpy()
    assert np.isnan(Kn[2]).all() and np.isnan(Kn[:, 2]).all() and np.isfinite(Kn[:2, :2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
def test_assembly_exp_accuracy(engine, mode):
    """The table-based exp() of the two kernel-assembly kernels (csrc/sgp_common.hpp: sgp_exp_tab -- 2^k T[j] (1 + q(r)), 32-entry
    table in LDS, one rounding after the table value) over its whole range, read back from the K'_fu block that kfu_assemble_kernel
    (fp64 contraction) and kfu_digits_kernel<.., true> (integer contraction) write: k'(x_n, z_0) = exp(-x_n^2 / 2) with z_0 = 0.
    <= 1.5 ulp against numpy's libm exp, exact 1 at 0, clean underflow, NaN stays NaN; both kernels write the same bits."""
    t = np.concatenate([np.linspace(0.0, 40.0, 3000), np.linspace(40.0, 744.0, 3000), [745.2, 760.0, 1.0e4]])
    x = np.sqrt(2.0 * t)
    N, M = x.size, 2
    X = dev(x[:, None], engine)
    y = dev(np.zeros(N), engine)
    Z = dev(np.array([[0.0], [np.nan]]), engine)
    prev = engine.lib.sgp_set_contraction(mode)
    try:
        kfu = engine.kfu_buffer(N, M)
        engine.suffstats(X, y, Z, [1.0], 1.0, "rbf", kfu=kfu)
        assert engine.lib.sgp_contraction_last() == (1 if mode else 0)
    finally:
        engine.lib.sgp_set_contraction(prev)
    K = kfu.view(-1, 128)[:N, :M].cpu().numpy()
    got, ref = K[:, 0], np.exp(-0.5 * (x * x))
    assert got[0] == 1.0
    big = ref > 1e-300
    rel = float(np.max(np.abs(got[big] - ref[big]) / ref[big]))
    ulps = float(np.max(np.abs(got[big] - ref[big]) / np.spacing(ref[big])))
    assert ulps <= 1.5 and rel < 2.5e-16, (ulps, rel)
    assert np.all(np.abs(got[~big] - ref[~big]) <= 1e-300) and np.all(np.isfinite(got)) and np.all(got >= 0.0)
    assert np.isnan(K[:, 1]).all()          # a NaN inducing input: NaN kernel values, never k = 0
    if mode == 2:
        kfu0 = engine.kfu_buffer(N, M)
        p0 = engine.lib.sgp_set_contraction(0)
        try:
            engine.suffstats(X, y, Z, [1.0], 1.0, "rbf", kfu=kfu0)
        finally:
            engine.lib.sgp_set_contraction(p0)
        a, b = kfu0.view(-1, 128)[:N, :1].cpu().numpy(), K[:, :1]
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_two_ranks_share_the_gpu_real_engine_matches_one_rank():
    """The multi-rank path on hardware, as far as a 1-GPU box allows: bench.py under torch.distributed.run with two
    ranks on cuda:0 (gloo carries the all-reduce of the packed statistics and of the gradients; RCCL refuses duplicate
    devices), HIP engine in both processes, against the same job in one process -- F to 1e-9 relative (the shards' Phi are
    summed in another order, and W = L^-1 Phi L^-T carries that rounding through cond(K_uu): 4e-11 observed), the leapfrog
    path exercised as well.  (Throughput of such a run means nothing.)"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    rows = 131072
    # --full: config.allreduce_ms (the packed all-reduce timed alone) is one of the extra measurements
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--rows", str(rows),
            "--full"]
    one = subprocess.run(base, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert one.returncode == 0, one.stderr[-2000:]
    r1 = json.loads(one.stdout.strip().splitlines()[-1])
    # bench.py's own launcher (`python bench.py --gpus 2`, what the driver's SCALE command runs): it starts the two ranks
    env = dict(os.environ, SGP_BENCH_BACKEND="gloo", SGP_BENCH_SHARE_GPU="1")
    env.pop("WORLD_SIZE", None)
    two = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert two.returncode == 0, two.stderr[-3000:]
    r2 = json.loads([ln for ln in two.stdout.strip().splitlines() if ln.startswith("{")][-1])
    assert r2["n_gpus"] == 2 and r2["config"]["ranks"] == 2 and r2["config"]["rows_per_rank"] == rows // 2
    # both jobs contract on the integer matrix cores (65536 rows x 1024^2 >= 2^32 per rank): the shards' statistics add up across ranks
    assert r1["config"]["contraction"].startswith("int8") and r2["config"]["contraction"].startswith("int8")
    assert abs(r2["F"] - r1["F"]) < 1e-9 * abs(r1["F"]), (r1["F"], r2["F"])
    assert r2["leapfrog_per_s"] > 0 and r2["value"] > 0
    assert r2["config"]["allreduce_ms"] > 0 and r2["config"]["collectives_per_eval"] == 1.0
    assert r2["config"]["allreduce_bytes"] == 8 * (1024 * 1025 // 2 + 1024 + 2)
    # the streaming-order guard on two ranks: at a long lengthscale x small noise BOTH ranks must decide, from the replicated tail and
    # the all-reduced statistics, to repeat the evaluation in the whitened order -- a rank deciding otherwise would leave the other
    # one alone in its all-reduce (the job would hang, not fail).  Same F as the one-process job, which repeats as well.
    hard = ["--ls", "6.0", "--sig-n", "0.03"]
    one_h = subprocess.run(base + hard, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert one_h.returncode == 0, one_h.stderr[-2000:]
    h1 = json.loads(one_h.stdout.strip().splitlines()[-1])
    two_h = subprocess.run(base + hard + ["--gpus", "2"], capture_output=True, text=True, timeout=1200, cwd=ROOT, env=env)
    assert two_h.returncode == 0, two_h.stderr[-3000:]
    h2 = json.loads([ln for ln in two_h.stdout.strip().splitlines() if ln.startswith("{")][-1])
    g1, g2 = h1["config"]["streaming_guard"], h2["config"]["streaming_guard"]
    assert g1["repeats_in_whitened_order"] > 0 and g2["repeats_in_whitened_order"] > 0, (g1, g2)
    assert g1["direct_whitened_evaluations"] == g2["direct_whitened_evaluations"] > 0        # the episode continues without streaming attempts
    assert g1["estimate_per_datum"] > g1["tolerance_per_datum"] and g2["estimate_per_datum"] > g2["tolerance_per_datum"]
    assert abs(h2["F"] - h1["F"]) < 1e-9 * abs(h1["F"]), (h1["F"], h2["F"])
    assert r1["config"]["streaming_guard"]["repeats_in_whitened_order"] == 0      # the benchmark's own theta never repeats
    # and without the sharing override a 1-GPU box must refuse, loudly, instead of printing n_gpus: 1
    import torch
    if torch.cuda.device_count() < 2:
        env2 = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "SGP_BENCH_SHARE_GPU", "SGP_BENCH_BACKEND")}
        bad = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env2)
        assert bad.returncode != 0 and "2 ranks" in bad.stderr and not bad.stdout.strip().startswith("{"), (bad.stdout, bad.stderr[-500:])


@pytest.mark.gpu
def test_bench_dump_outputs_holds_the_last_timed_step(tmp_path):
    """bench.py --dump-outputs on the device: --steps timed evaluations, ms_per_step their mean, and the dumped F the one the result
    line reports (the last timed evaluation's); the gradient files are finite and of the workload's dimension."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--cpu-sample", "0", "--rows", "131072",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert abs(res["ms_per_step"] - 1e3 / res["value"]) < 1e-9 * res["ms_per_step"]
    F = np.load(str(out / "F.npy"))
    assert F.dtype == np.float64 and F.shape == (1,) and F[0] == res["F"]
    g = np.load(str(out / "grad_ls.npy"))
    assert g.shape == (res["config"]["d"],) and np.isfinite(g).all()
    assert sum(os.path.getsize(str(out / f)) for f in os.listdir(out)) < 64 << 20


@pytest.mark.gpu
def test_bench_full_adds_the_extra_measurements_to_the_same_timed_steps():
    """A plain bench.py run prints the headline, leapfrog_per_s, F and the configuration only; --full times the same steps on the
    same seeded inputs and adds the kernel rooflines, the guard's fallback orders and the trained-theta leapfrogs (the CPU
    baseline is skipped here: --cpu-sample 0)."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--cpu-sample", "0", "--rows", "131072"]
    runs = {}
    for name, extra in (("plain", []), ("full", ["--full"])):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = json.loads(r.stdout.strip().splitlines()[-1])
    plain, full = runs["plain"], runs["full"]
    moved = ("roofline", "roofline_fp64_contraction", "roofline_leapfrog", "assembly", "leapfrog_per_s_trained_theta", "cpu_baseline")
    for res in (plain, full):
        assert res["metric"] == "ELBO evals/sec" and res["unit"] == "evals/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
        assert res["steps"] == 2 and res["warmup"] == 1 and abs(res["ms_per_step"] - 1e3 / res["value"]) < 1e-9 * res["ms_per_step"]
        assert res["leapfrog_per_s"] > 0 and res["config"]["contraction"].startswith("int8")
        assert res["config"]["streaming_guard"]["repeats_in_whitened_order"] == 0
    assert not any(k in plain for k in moved)
    assert "whitened_order" not in plain["config"]["streaming_guard"] and plain["config"]["allreduce_ms"] is None
    assert abs(full["F"] - plain["F"]) < 1e-12 * abs(plain["F"])
    assert full["roofline"]["ms"] > 0 and full["roofline"]["kernel"].startswith("sgp::i8_syrk_tile_kernel")
    assert full["roofline_fp64_contraction"]["ms"] > 0 and full["roofline_leapfrog"]["ms"] > 0 and full["assembly_digits"]["ms"] > 0
    assert full["config"]["streaming_guard"]["whitened_order"]["ms_per_evaluation"] > 0
    assert full["config"]["streaming_guard"]["extended_order"]["ms_per_leapfrog"] > 0
    assert full["leapfrog_per_s_trained_theta"]["parity"] > 0 and "cpu_baseline" not in full


@pytest.mark.gpu
def test_pass1_head_tail_blocks_and_side_stream_assembly(engine):
    """The A/B knob sgp_set_asm_overlap (pass 1 as head block + tail block, the tail's kernel assembly on the library's side stream
    beside the head's contraction): mode 1 (overlapped) and mode 2 (the same blocks enqueued serially) must agree bit for bit, and
    both with the one-block default to rounding -- on a shard big enough for the tapered plan (400k x 512) and with a caller-owned
    K'_fu, which pass 2 then reads: its gradients must not depend on the mode either."""
    import ggp_amd
    g = torch.Generator().manual_seed(11)
    N, M, d = 400_000, 512, 4
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    Xd, yd, Zd = X.to(engine.device), y.to(engine.device), Z.to(engine.device)
    ls = [0.6, 0.7, 0.5, 0.8]  # short lengthscales: a well-conditioned K_uu, so F itself can be compared to rounding
    out = {}
    prev = engine.lib.sgp_set_contraction(0)  # the head / tail blocks belong to the fp64 contraction (the integer one would bypass them)
    try:
        for mode in (0, 1, 2, 1):
            engine.lib.sgp_set_asm_overlap(mode)
            kfu = engine.kfu_buffer(N, M)
            st = engine.suffstats(Xd, yd, Zd, ls, 1.3, "rbf", kfu=kfu).clone()
            cb = ggp_amd.CollapsedBound(Xd, yd, jitter=1e-6, engine=engine, form="streaming")
            F, gr = cb.value_and_grad(Zd, ls, 1.3, 0.05, want_gz=False)
            out.setdefault(mode, []).append((st, kfu.clone(), F, gr["ls"].clone(), gr["sf2"], gr["s2"]))
            del kfu
            assert engine.lib.sgp_contraction_last() == 0
    finally:
        engine.lib.sgp_set_asm_overlap(-1)
        engine.lib.sgp_set_contraction(prev)
    (s0, k0, F0, g0, a0, b0), (s1, k1, F1, g1, a1, b1), (s2, k2, F2, g2, a2, b2) = out[0][0], out[1][0], out[2][0]
    assert torch.equal(k0, k1) and torch.equal(k1, k2)                       # K'_fu itself does not depend on the blocks
    assert torch.equal(s1, s2) and F1 == F2 and torch.equal(g1, g2) and (a1, b1) == (a2, b2)
    assert torch.equal(out[1][1][0], s1) and out[1][1][2] == F1              # and run to run
    assert float((s0 - s1).abs().max()) < 1e-12 * float(s0.abs().max())
    assert abs(F0 - F1) < 1e-11 * abs(F0) and float((g0 - g1).abs().max()) < 1e-9 * float(g0.abs().max())


@pytest.mark.gpu
def test_conditioning_gate_of_the_explicit_inverse_path(engine):
    """sgp_kuu_factor refuses a K_uu whose condition estimate trace(K) / min pivot exceeds the limit (default 1e13): downstream the explicit L^-1 would turn the bound into noise (profiles/r03_co2_m480_chol_ab.json: cond 1e15,
    F off by 6e3 where LAPACK is smooth), and a sampler must see a zero-density region rather than a spurious spike.
    A well-conditioned matrix passes; with the gate switched off the same ill-conditioned matrix factors (as in LAPACK)."""
    import ggp_amd
    z = torch.linspace(0.0, 52.0, 300, dtype=torch.float64)[:, None]
    ok = engine.kuu(dev(z.numpy(), engine), [0.5], 2.0, 1e-6, "rbf")          # cond ~ 1e7
    bad = engine.kuu(dev(z.numpy(), engine), [3.0], 2.0e6, 1e-6, "rbf")       # lambda_max ~ 5e8 against the 1e-6 jitter: cond ~ 1e14-1e15
    assert int(engine.kuu_factor(ok)[1].cpu()[0]) == 0
    info = int(engine.kuu_factor(bad)[1].cpu()[0])
    assert 1 <= info <= 300
    assert np.linalg.cholesky(bad.cpu().numpy()) is not None                   # LAPACK itself does not fail here
    try:
        engine.lib.sgp_set_cond_limit(0.0)
        assert int(engine.kuu_factor(bad)[1].cpu()[0]) == 0
    finally:
        engine.lib.sgp_set_cond_limit(-1.0)
    assert int(engine.kuu_factor(bad)[1].cpu()[0]) == info
    # through the model layer: the NUTS target reports -inf there, never a finite garbage value
    X = torch.linspace(0.0, 52.0, 634, dtype=torch.float64)[:, None]
    yv = torch.sin(X[:, 0])
    cb = ggp_amd.CollapsedBound(dev(X.numpy(), engine), dev(yv.numpy(), engine), jitter=1e-6, engine=engine, form="whitened")
    cb.fused = False
    tgt = ggp_amd.HmcTarget(cb, dev(z.numpy(), engine))
    lp, _ = tgt.logp_and_grad([math.log(3.0), 0.5 * math.log(2.0e6), math.log(0.01)])
    assert lp == -math.inf
    lp2, _ = tgt.logp_and_grad([math.log(0.5), 0.0, math.log(0.1)])
    assert math.isfinite(lp2)


@pytest.mark.gpu
def test_conditioning_gate_accepts_a_well_posed_large_amplitude_problem(engine):
    """unnormalised targets (CO2 in ppm) put the amplitude at ~1e4; with M = 1000 well-spread inducing inputs and ONE
    near-duplicate pair (min pivot ~ the jitter) round 3's estimate trace(K) / min pivot = M sf2 / J = 1e13+ refused a matrix whose
    condition number is ~2 sf2 / J = 2e10 -- which LAPACK, the reference's substitution solves and the single-launch path evaluate.
    The column-norm estimate can only undershoot cond: the matrix passes, and the bound still agrees with the oracle."""
    import ggp_amd
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(3)
    M, N, d = 1000, 4000, 2
    X = torch.rand(N, d, dtype=torch.float64, generator=g) * 40.0
    y = 100.0 * torch.sin(X[:, 0]) * torch.cos(0.5 * X[:, 1]) + torch.randn(N, dtype=torch.float64, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    Z[1] = Z[0] + 1e-9                                     # one near-duplicate pair
    sf2, ls = 2.0e4, [0.7, 0.7]                              # M sf2 / jitter = 2e13 > the 1e13 limit; cond ~ 4e10
    K = engine.kuu(dev(Z.numpy(), engine), ls, sf2, 1e-6, "rbf")
    assert int(engine.kuu_factor(K)[1].cpu()[0]) == 0
    cb = ggp_amd.CollapsedBound(dev(X.numpy(), engine), dev(y.numpy(), engine), jitter=1e-6, engine=engine)
    cb.fused = False
    F, parts = cb.value(dev(Z.numpy(), engine), ls, sf2, 1.0)
    F_ref = O.vfe_pymc3_order_chunked(X, y, Z, torch.tensor(ls, dtype=torch.float64), math.sqrt(sf2), 1.0, 1e-6)
    assert abs(F - F_ref) < 1e-6 * abs(F_ref), (F, F_ref)


@pytest.mark.gpu
def test_mixture_predictive_batched_over_the_samples(engine):
    """sgp_mixture_predict (row f-2: eight theta samples per chain of launches, PSD gates in one dataflow launch) against the
    oracle's predictive sample by sample, against the per-sample loop of the reference (model.batched_mixture = False), with
    N > 8192 (two row chunks of the train side), T not a multiple of 64, 11 samples (two batches) and one sample whose K_uu is
    hopeless (amplitude 1e5, lengthscale 30 against the 1e-6 jitter): both paths drop exactly that one."""
    import ggp_amd
    from oracle import vfe_oracle as O
    from ggp_amd.hmc import Trace
    g = torch.Generator().manual_seed(8)
    N, M, T, d = 9000, 70, 333, 3
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X[:, 0]) * torch.cos(X[:, 1]) + 0.3 * X[:, 2] + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Xt = torch.randn(T, d, dtype=torch.float64, generator=g)
    Z0 = X[torch.randperm(N, generator=g)[:M]].clone()
    Xd, yd, Xtd, Zd = X.to(engine.device), y.to(engine.device), Xt.to(engine.device), Z0.to(engine.device)
    # lengthscales below the typical inducing-point spacing: K_uu well conditioned, so 1e-8 against the (streaming-order) oracle is
    # a statement about the kernels, not about cond(K_uu) eps
    rows = [{"ls": np.array([0.6 + 0.02 * i, 0.8 - 0.01 * i, 0.7]), "sig_f": 1.0 + 0.05 * i, "sig_n": 0.3 + 0.02 * i} for i in range(11)]
    rows[4] = {"ls": np.array([30.0, 30.0, 30.0]), "sig_f": 1.0e5, "sig_n": 0.3}
    for kern, kid in (("rbf", 0), ("matern32", 1)):
        r = engine.mixture_predict(Xd, yd, Xtd, Zd, [q["ls"] for q in rows], [q["sig_f"] ** 2 for q in rows], [q["sig_n"] ** 2 for q in rows],
                                   jitter=1e-6, kernel=kern, full_cov=True, gate_jitter=1e-4)
        info, gate = r["info"].cpu().tolist(), r["gate"].cpu().tolist()
        bad = [i for i, v in enumerate(info) if v != 0]
        if kid == 0:   # RBF: numerically rank-deficient at lengthscale 30 -> refused (LAPACK itself fails at pivot 41)
            assert bad == [4] and 1 <= info[4] <= M
        else:          # the rougher Matern-3/2 profile keeps K_uu factorable there; no OTHER sample may be flagged
            assert set(bad) <= {4}
        for i in (0, 7, 8, 10):  # first / last of both batches
            q = rows[i]
            mu, cov = O.predict(Xt, X, y, Z0, torch.as_tensor(q["ls"]), q["sig_f"] ** 2, q["sig_n"] ** 2, 1e-6, kernel_id=kid, full_cov=True)
            assert float((r["mean"][i].cpu() - mu).abs().max()) < 1e-8
            assert float((r["cov"][i].cpu() - cov).abs().max()) < 1e-8
            assert float((r["var"][i].cpu() - torch.diagonal(cov)).abs().max()) < 1e-8
            assert gate[i] == 0
        val = engine.mixture_predict(Xd, yd, Xtd, Zd, [q["ls"] for q in rows], [q["sig_f"] ** 2 for q in rows], [q["sig_n"] ** 2 for q in rows],
                                     jitter=1e-6, kernel=kern)
        assert val["cov"] is None and torch.equal(val["mean"][0], r["mean"][0]) and torch.equal(val["var"][10], r["var"][10])
    # the model-level list of predictives, batched and in the reference's loop
    model = ggp_amd.BayesianSparseGPR_HMC(Xd, yd, ggp_amd.GaussianLikelihood(), Z0, engine=engine, jitter=1e-6)
    trace = Trace(rows, {"step_size": np.zeros(len(rows))})
    pb = ggp_amd.mixture_posterior_predictive(model, Xtd, trace)
    assert abs(float(model.likelihood.noise) - rows[-1]["sig_n"] ** 2) < 1e-12      # left at the last sample, as the loop does
    model.batched_mixture = False
    pl = ggp_amd.mixture_posterior_predictive(model, Xtd, trace)
    assert len(pb) == len(pl) == 10
    for a, b in zip(pb, pl):
        assert float((a.loc - b.loc).abs().max()) < 1e-8 and float((a.covariance_matrix - b.covariance_matrix).abs().max()) < 1e-8
    yt = torch.sin(Xt[:, 0]) * torch.cos(Xt[:, 1]) + 0.3 * Xt[:, 2]
    assert abs(ggp_amd.nlpd_mixture(pb, yt, torch.tensor([1.0])) - ggp_amd.nlpd_mixture(pl, yt, torch.tensor([1.0]))) < 1e-7


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,T,d,S", [(50, 5, 1, 1, 1), (8193, 129, 65, 2, 3), (700, 64, 64, 5, 8), (130, 128, 200, 3, 9)])
def test_mixture_predictive_edge_shapes(engine, N, M, T, d, S):
    """sgp_mixture_predict at the edges of its tiling: a single test row, one row past the 8192-row training chunk, M one past a
    128 boundary, exact multiples of 64, more samples than one batch -- mean / variance / covariance against the oracle per sample."""
    from oracle import vfe_oracle as O
    g = torch.Generator().manual_seed(N + M + T)
    X = torch.randn(N, d, dtype=torch.float64, generator=g)
    y = torch.sin(X.sum(1)) + 0.1 * torch.randn(N, dtype=torch.float64, generator=g)
    Xt = torch.randn(T, d, dtype=torch.float64, generator=g)
    Z = (X[torch.randperm(N, generator=g)[:M]] if M <= N else torch.randn(M, d, dtype=torch.float64, generator=g)).clone()
    # lengthscales below the inducing-point spacing (129 points in 2-D sit closer than 70 in 3-D): a test of the tiling, not of
    # cond(K_uu) eps -- at ls 0.5-0.8 the d = 2 case differs from the (streaming-order) oracle by 5e-7 everywhere.  That difference is
    # the oracle's: against long double the kernels stay within a few 1e-11 of the condition scale at such a cell (300-65-2-rbf of
    # tests/test_stream_predict_gpu.py), where the streaming-order float64 evaluation is 1e-9 of it away
    ls = (0.5 + 0.3 * torch.rand(S, d, dtype=torch.float64, generator=g)) * (0.4 if d <= 2 else 1.0)
    sf2 = 0.8 + 0.5 * torch.rand(S, dtype=torch.float64, generator=g)
    s2 = 0.05 + 0.1 * torch.rand(S, dtype=torch.float64, generator=g)
    D = lambda t: t.to(engine.device).contiguous()  # noqa: E731
    r = engine.mixture_predict(D(X), D(y), D(Xt), D(Z), ls.tolist(), sf2.tolist(), s2.tolist(), jitter=1e-6, kernel="rbf", full_cov=True,
                               gate_jitter=1e-4)
    assert r["info"].cpu().tolist() == [0] * S and r["gate"].cpu().tolist() == [0] * S
    for k in range(S):
        mu, cov = O.predict(Xt, X, y, Z, ls[k], float(sf2[k]), float(s2[k]), 1e-6, full_cov=True)
        assert float((r["mean"][k].cpu() - mu).abs().max()) < 1e-8, k
        assert float((r["cov"][k].cpu() - cov).abs().max()) < 1e-8, k
        assert float((r["var"][k].cpu() - torch.diagonal(cov)).abs().max()) < 1e-8, k
