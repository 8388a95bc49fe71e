"""GPU: saf_query_scan and saf_query_topk on rows that hold an inf or a NaN -- on every route of the dispatch, under every
normalisation mode and epilogue, through the C ABI (ctypes), with `out` and `out_last` in one call and `out = NULL` in another.

The rule (include/saf.h; tests/text_scan_reference.py restates it; tests/test_text_scan_bad_rows_host.py shows that the oracle alone
obeys it):
  * SAF_NORM_L2: a bad row is the all-zero row on every route -- 0.0 in every column (scores), 1 / L (softmax; fp32(1) / fp32(L)
    within one ulp, the bar include/saf.h sets for the top-k's probabilities), 0.0 (surgery); top-k: labels 0 .. k - 1, probability
    1 / L each.  A bad row 0 gives the surgery weights of the zero row.
  * SAF_NORM_NONE, SAF_NORM_L2_CLAMP: every column of a bad row is not finite, as the oracle's is; where both are infinite the sign
    agrees (NaN against infinity is not compared: the split scans cut an inf into hi = inf and lo = NaN).  Top-k: a row all of whose
    scores the oracle has as NaN reports label -1 at probability 0; any other bad row labels in [-1, L), none twice.
  * Every mode, epilogue and route: out_last is the last column of the same call bit for bit; every good row is bit for bit what the
    same call gives on the volume without the bad rows, and within the project's tolerance (rtol 1e-4, atol 2e-6) of the oracle.

Routes: tests/text_scan_reference.py's ROUTES, named after tests/test_query_outputs.py's CASES with "matrix" told apart into the
exact-fp32 scan, the split scan and its 16-bit form.  Each test first checks that the documented conditions of the dispatch give the
route the case is named after, and test_dispatch_launches_the_kernels_of_each_route reads the kernels that really ran from the
profiler's trace: a quiet change of the dispatch fails there.

Shapes: 1000 rows = 31 whole 32-row tiles and a ragged one of 8; 40 rows (one case per route) = one whole tile and 8 rows."""
import re

import numpy as np
import pytest
import torch

import text_scan_reference as R
from spatially_aware_ai_amd import _abi

pytestmark = pytest.mark.gpu

L2, NONE, CLAMP = _abi.SAF_NORM_L2, _abi.SAF_NORM_NONE, _abi.SAF_NORM_L2_CLAMP


def _err():
    from spatially_aware_ai_amd._lib import lib

    return lib().saf_last_error().decode()


def _one_ulp(got, want):
    """every fp32 value of `got` within one unit in the last place of the fp32 value `want`"""
    want = np.float32(want)
    return bool((np.abs(got.astype(np.float64) - np.float64(want)) <= np.float64(np.spacing(want))).all())


def _check_bad(what, got, want, nl, epi, mode):
    """a bad row's outputs `got` [b, L] (or [b]: the last column) against the rule and the oracle's `want` of the same shape"""
    assert not (got == np.float32(R.POISON)).any(), f"{what}: an output of a bad row was not written"
    if mode == L2:
        zero = R.zero_row(nl, epi)
        assert (want == np.float32(zero)).all(), f"{what}: the oracle's bad rows are not the zero row"
        if epi == _abi.SAF_Q_SOFTMAX:
            exact = int((got == np.float32(1.0) / np.float32(nl)).sum())
            print(f"{what}: softmax of a bad row: {exact} of {got.size} values are fp32(1) / fp32({nl}) exactly")
            assert _one_ulp(got, np.float32(1.0) / np.float32(nl)), f"{what}: a bad row's softmax is not 1 / L in every column"
        else:
            assert (got == 0.0).all(), f"{what}: a bad row must give 0 in every column, got {got[got != 0.0][:4]}"
    else:
        assert not np.isfinite(want).any(), f"{what}: the oracle's outputs of a bad row are not finite without nan_to_num"
        assert not np.isfinite(got).any(), f"{what}: a finite output on a bad row where the oracle has none"
        both = np.isinf(got) & np.isinf(want)
        assert np.array_equal(np.sign(got[both]), np.sign(want[both])), f"{what}: an infinity of the other sign than the oracle's"


def _run_scan_case(oracle, monkeypatch, case, n, mode, row0=False, epilogues=R.EPILOGUES):
    route, d, nl, dt, padded, env = case
    if env is None:
        monkeypatch.delenv("SAF_Q_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SAF_Q_SPLIT", env)
    good, bad, text, is_bad = R.scene(n, d, nl, dt, row0)
    gd, bd, text_d = R.on_device(good, padded), R.on_device(bad, padded), text.cuda()
    stride = d + 8 if padded else d
    assert bd.stride(0) == stride and gd.stride(0) == stride
    aligned = bd.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 0
    R.check_route(route, R.expected_kernels(dt, stride, d, nl, _abi.SAF_Q_SOFTMAX, True, aligned, env))
    bad_np = is_bad.numpy()
    keep = ~bad_np
    for epi, scale in epilogues:
        what = f"{R.route_id(case)}, {n} rows, mode {R.MODE_NAMES[mode]}, epilogue {epi}" + (", bad row 0" if row0 else "")
        want = R.truth(oracle, n, d, nl, dt, row0, epi, scale, mode)
        res = {}
        for vol, fd in (("bad", bd), ("good", gd)):
            rc, out, last = R.scan(fd, text_d, epi, scale, mode, True, True)
            assert rc == 0, f"{what} ({vol}): rc {rc}: {_err()}"
            rc, none, only = R.scan(fd, text_d, epi, scale, mode, False, True)
            assert rc == 0 and none is None, f"{what} ({vol}, out = NULL): rc {rc}: {_err()}"
            res[vol] = (out.cpu().numpy(), last.cpu().numpy(), only.cpu().numpy())
        out, last, only = res["bad"]
        g_out, g_last, g_only = res["good"]
        # ---- one call: out_last is its last column
        assert np.array_equal(R.bits(last), R.bits(out[:, nl - 1])), f"{what}: out_last is not the last column of the same call"
        # ---- good rows: untouched by the bad rows, and the oracle's
        assert not (out[keep] == np.float32(R.POISON)).any() and not (only[keep] == np.float32(R.POISON)).any(), f"{what}: not written"
        assert np.array_equal(R.bits(out[keep]), R.bits(g_out[keep])), f"{what}: a bad row changed a good row's output"
        assert np.array_equal(R.bits(last[keep]), R.bits(g_last[keep])), f"{what}: a bad row changed a good row's out_last"
        assert np.array_equal(R.bits(only[keep]), R.bits(g_only[keep])), f"{what}: a bad row changed a good row's out_last (out = NULL)"
        err = np.abs(out[keep].astype(np.float64) - want[keep])
        print(f"{what}: good rows max abs err {err.max():.3g}, max err / (atol + rtol |want|) "
              f"{(err / (R.ATOL + R.RTOL * np.abs(want[keep]))).max():.3g}; bad rows NaN {int(np.isnan(out[bad_np]).sum())}, "
              f"inf {int(np.isinf(out[bad_np]).sum())} of {out[bad_np].size}")
        np.testing.assert_allclose(out[keep], want[keep], rtol=R.RTOL, atol=R.ATOL, err_msg=what)
        np.testing.assert_allclose(only[keep], want[keep, nl - 1], rtol=R.RTOL, atol=R.ATOL, err_msg=what + " (out = NULL)")
        # ---- bad rows: the rule
        _check_bad(what, out[bad_np], want[bad_np], nl, epi, mode)
        _check_bad(what + " (out = NULL)", only[bad_np], want[bad_np, nl - 1], nl, epi, mode)


@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
@pytest.mark.parametrize("case", R.ROUTES, ids=R.route_id)
def test_bad_rows_on_every_route(oracle, monkeypatch, case, mode):
    _run_scan_case(oracle, monkeypatch, case, R.N_MAIN, mode)


@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
@pytest.mark.parametrize("case", R.ONE_PER_ROUTE, ids=R.route_id)
def test_bad_rows_in_a_tile_and_eight_rows(oracle, monkeypatch, case, mode):
    """40 rows: bad rows in the only whole tile and at rows 32, 36 and 39 of the ragged one"""
    _run_scan_case(oracle, monkeypatch, case, R.N_SMALL, mode)


@pytest.mark.parametrize("case", R.ONE_PER_ROUTE, ids=R.route_id)
def test_bad_row_zero_gives_the_zero_rows_surgery_weights(oracle, monkeypatch, case):
    """SAF_NORM_L2, surgery, row 0 bad: the weights are the zero row's (uniform) on every route -- they come from the one-wave-per-row
    kernel whatever scans the volume -- so every good row is bit for bit what the volume with an all-zero row 0 gives"""
    _run_scan_case(oracle, monkeypatch, case, R.N_MAIN, L2, row0=True, epilogues=((_abi.SAF_Q_SURGERY, 1.0),))


# ------------------------------------------------------------------------------------------ top-k
TOPK_SCALE = 100.0


@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
@pytest.mark.parametrize("case", R.TOPK_ROUTES, ids=R.route_id)
def test_topk_on_bad_rows(oracle, monkeypatch, case, mode):
    """saf_query_topk, k = 1, 5, 8, with and without out_prob.  Good rows against the oracle: the device's cosine is held to the
    project's tolerance and the scale multiplies it, so the label the device ranks j-th has an oracle score within
    2 * scale * (atol + rtol |cos|) of the oracle's j-th best (two labels swap only when they are that close), and its probability is
    the oracle's softmax of that label within the tolerance."""
    route, d, nl, dt = case
    monkeypatch.delenv("SAF_Q_SPLIT", raising=False)
    n = R.N_MAIN
    good, bad, text, is_bad = R.scene(n, d, nl, dt)
    gd, bd, text_d = good.cuda(), bad.cuda(), text.cuda()
    R.check_route(route, R.expected_topk_kernels(dt, d, d, nl, bd.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 0))
    bad_np = is_bad.numpy()
    keep = ~bad_np
    s = R.truth(oracle, n, d, nl, dt, False, _abi.SAF_Q_SCORES, TOPK_SCALE, mode).astype(np.float64)
    p = R.truth(oracle, n, d, nl, dt, False, _abi.SAF_Q_SOFTMAX, TOPK_SCALE, mode).astype(np.float64)
    if mode == L2:
        assert (s[bad_np] == 0).all()
    else:
        assert not np.isfinite(s[bad_np]).any(), "the oracle's scores of a bad row are not finite without nan_to_num"
    all_nan = np.isnan(s).all(axis=1)
    assert not all_nan[keep].any() and (mode == L2 or all_nan[bad_np].any())
    best = -np.sort(-s[keep], axis=1)
    rows = np.arange(n)[keep]
    for k in (1, 5, 8):
        for want_prob in (True, False):
            what = f"{R.route_id(case)}, mode {R.MODE_NAMES[mode]}, k {k}, out_prob {'given' if want_prob else 'NULL'}"
            rc, idx, prob = R.topk(bd, text_d, TOPK_SCALE, mode, k, want_prob)
            assert rc == 0, f"{what}: rc {rc}: {_err()}"
            rc, g_idx, g_prob = R.topk(gd, text_d, TOPK_SCALE, mode, k, want_prob)
            assert rc == 0, f"{what} (good volume): rc {rc}: {_err()}"
            idx, g_idx = idx.cpu().numpy(), g_idx.cpu().numpy()
            assert not (idx == -7).any(), f"{what}: a label was not written"
            # ---- good rows
            assert np.array_equal(idx[keep], g_idx[keep]), f"{what}: a bad row changed a good row's labels"
            gi = idx[keep]
            assert ((gi >= 0) & (gi < nl)).all() and all(len(set(r)) == k for r in gi.tolist()), f"{what}: good rows' labels"
            picked = s[rows[:, None], gi]
            gap = np.abs(picked - best[:, :k])
            bound = 2 * TOPK_SCALE * (R.ATOL + R.RTOL * np.abs(best[:, :k]) / TOPK_SCALE)
            differs = int((gi != R.stable_topk(s[keep], k).numpy()).sum())
            print(f"{what}: {differs} of {gi.size} labels differ from the oracle's stable top-k; rank score gap max {gap.max():.3g} "
                  f"(bound {bound.min():.3g} at the least)")
            assert (gap <= bound).all(), f"{what}: a good row's j-th label does not have the j-th best score"
            if want_prob:
                prob, g_prob = prob.cpu().numpy(), g_prob.cpu().numpy()
                assert not (prob == np.float32(R.POISON)).any(), f"{what}: a probability was not written"
                assert np.array_equal(R.bits(prob[keep]), R.bits(g_prob[keep])), f"{what}: a bad row changed a good row's probabilities"
                np.testing.assert_allclose(prob[keep], p[rows[:, None], gi], rtol=R.RTOL, atol=R.ATOL, err_msg=what)
            # ---- bad rows
            bi = idx[bad_np]
            if mode == L2:
                assert np.array_equal(bi, np.tile(np.arange(k, dtype=np.int32), (bi.shape[0], 1))), f"{what}: a bad row's labels are not 0 .. k - 1"
                if want_prob:
                    assert _one_ulp(prob[bad_np], np.float32(1.0) / np.float32(nl)), f"{what}: a bad row's probabilities are not 1 / L"
            else:
                nan_rows = all_nan[bad_np]
                assert (bi[nan_rows] == -1).all(), f"{what}: a row of NaN scores must report label -1"
                if want_prob:
                    assert (prob[bad_np][nan_rows] == 0.0).all(), f"{what}: a row of NaN scores must report probability 0"
                assert ((bi >= -1) & (bi < nl)).all(), f"{what}: a bad row's label outside [-1, L)"
                for r in bi.tolist():
                    real = [l for l in r if l != -1]
                    assert len(set(real)) == len(real), f"{what}: a bad row reports a label twice: {r}"


# ------------------------------------------------------------------------------------------ which kernels ran
_KERNELS = ("query_kernel", "query_mfma_kernel", "query_split_kernel", "query_split16_kernel", "finish_rows_kernel", "topk_rows_kernel")
_KERNEL_RE = re.compile(r"\b(" + "|".join(_KERNELS) + r")\b")


def test_dispatch_launches_the_kernels_of_each_route(monkeypatch):
    """every route case, every epilogue, with `out` and with out = NULL, and every top-k case, on 40 good rows under one profiler
    session: the kernels of this library in the trace, in launch order, are those the documented conditions name
    (tests/text_scan_reference.py: expected_kernels)"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    plan, expected = [], []
    for case in R.ROUTES:
        route, d, nl, dt, padded, env = case
        good, _, text, _ = R.scene(R.N_SMALL, d, nl, dt)
        fd, text_d = R.on_device(good, padded), text.cuda()
        for epi, scale in R.EPILOGUES:
            for want_out in (True, False):
                plan.append((env, lambda fd=fd, text_d=text_d, epi=epi, scale=scale, want_out=want_out: R.scan(fd, text_d, epi, scale, L2, want_out, True)))
                kernels = R.expected_kernels(dt, fd.stride(0), d, nl, epi, want_out, fd.data_ptr() % 16 == 0, env)
                expected += [(k, f"{R.route_id(case)}, epilogue {epi}, out {'given' if want_out else 'NULL'}") for k in kernels]
    for case in R.TOPK_ROUTES:
        route, d, nl, dt = case
        good, _, text, _ = R.scene(R.N_SMALL, d, nl, dt)
        fd, text_d = good.cuda(), text.cuda()
        plan.append((None, lambda fd=fd, text_d=text_d: R.topk(fd, text_d, TOPK_SCALE, CLAMP, 5)))
        expected += [(k, R.route_id(case)) for k in R.expected_topk_kernels(dt, d, d, nl, fd.data_ptr() % 16 == 0)]
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for env, call in plan:
            if env is None:
                monkeypatch.delenv("SAF_Q_SPLIT", raising=False)
            else:
                monkeypatch.setenv("SAF_Q_SPLIT", env)
            assert call()[0] == 0, _err()
        torch.cuda.synchronize()
    events = sorted((e for e in prof.events() if e.device_type == DeviceType.CUDA), key=lambda e: e.time_range.start)
    ran = [m.group(1) for m in (_KERNEL_RE.search(e.name) for e in events) if m]
    print(f"{len(events)} device events in the trace, {len(ran)} kernels of the text scans; {len(expected)} expected")
    assert ran, "the profiler's trace holds no kernel of the text scans"
    for i, (k, what) in enumerate(expected):
        assert i < len(ran) and ran[i] == k, f"{what}: launch {i} should be {k}, the trace has {ran[i] if i < len(ran) else 'nothing'}"
    assert len(ran) == len(expected), f"{len(ran) - len(expected)} launches more than the conditions name: {ran[len(expected):][:6]}"
