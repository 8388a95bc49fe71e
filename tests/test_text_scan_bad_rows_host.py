"""CPU: what tests/test_text_scan_bad_rows.py holds the HIP scans to is what the reference does.  On the planted volumes of every
case of the device test (tests/text_scan_reference.py):

  * the oracle (oracle/saf_oracle.c) equals the float64 statement of the reference's lines;
  * the oracle alone satisfies the rule of include/saf.h: under SAF_NORM_L2 a bad row gives 0 (scores), 1 / L (softmax) and 0
    (surgery, the zero row's value) in every column, and uniform surgery weights when it is row 0; under SAF_NORM_NONE and
    SAF_NORM_L2_CLAMP every column of a bad row is not finite;
  * the planted rows are the only bad rows: rounded to the 16-bit dtypes the good rows stay finite and non-zero.

The oracle against the statement.  The oracle rounds each normalised feature and each score to fp32 where the statement keeps
float64: three roundings of 2^-24 on a cosine whose terms sum to at most |f^| |t| <= 1.5 in magnitude, 2.7e-7 at the worst.  Raw
scores (scale 3): 8e-7 absolute.  Softmax (scale 100): 2.7e-5 on a logit, twice that relative on a probability.  Surgery: the
weights move by 1e-6 relative, a weighted score and its mean by 5e-7 each.  HOST_RTOL = 6e-5 and HOST_ATOL = 1e-6 cover the three;
both are below the project's tolerance on the device scans (1e-4, 2e-6), which are compared with the oracle."""
import numpy as np
import pytest
import torch

import text_scan_reference as R
from spatially_aware_ai_amd import _abi

HOST_RTOL, HOST_ATOL = 6e-5, 1e-6

SCENES = sorted({(n, c[1], c[2], c[3], False) for c in R.ROUTES for n in (R.N_MAIN,)}
                | {(R.N_SMALL, c[1], c[2], c[3], False) for c in R.ONE_PER_ROUTE}
                | {(R.N_MAIN, c[1], c[2], c[3], True) for c in R.ONE_PER_ROUTE}
                | {(R.N_MAIN, c[1], c[2], c[3], False) for c in R.TOPK_ROUTES}, key=lambda s: (s[0], s[1], s[2], R.name(s[3]), s[4]))


def _id(s):
    return f"n{s[0]}-D{s[1]}-L{s[2]}-{R.name(s[3])}" + ("-row0" if s[4] else "")


def test_every_kind_at_a_tile_head_and_elsewhere():
    rows = R.bad_rows(R.N_MAIN)
    heads = {k for r, k in rows if r % 32 == 0}
    elsewhere = {k for r, k in rows if r % 32 != 0}
    assert heads == elsewhere == set(range(5))
    assert {r % 32 for r, _ in rows if r // 32 in (1, 16)} == {0, 1, 4, 16, 31}
    assert {992, 996, 999} <= {r for r, _ in rows} and all(r != 0 for r, _ in rows)
    small = R.bad_rows(R.N_SMALL)
    assert {r for r, _ in small} == {1, 4, 16, 31, 32, 36, 39} and {k for _, k in small} == set(range(5))


@pytest.mark.parametrize("sc", SCENES, ids=_id)
def test_planted_rows_are_the_only_bad_rows(sc):
    n, d, nl, dt, row0 = sc
    good, bad, text, is_bad = R.scene(n, d, nl, dt, row0)
    assert good.dtype == dt and bad.dtype == dt and int(is_bad.sum()) == len(R.bad_rows(n, row0))
    finite = torch.isfinite(bad.float()).all(dim=1)
    assert torch.equal(~finite, is_bad), "a bad row that was not planted, or a planted row that is finite"
    assert bool(torch.isfinite(good.float()).all())
    keep = ~is_bad
    assert bool((good.float()[keep] != 0).all()), "a good row's element rounded to zero"
    assert torch.equal(good[keep].view(torch.int16 if dt != R.F32 else torch.int32), bad[keep].view(torch.int16 if dt != R.F32 else torch.int32))
    if dt == R.F16:
        assert float(good.float()[keep].abs().min()) >= 2.0 ** -14, "an fp16 denormal among the good rows"
    if row0:
        assert bool(is_bad[0]) and bool((good[0] == 0).all())
    norms = good.double()[keep].norm(dim=-1)
    assert float(norms.min()) < 0.1 < 0.4 < float(norms.max()) < 1.51,"rows on both sides of the clamp, none beyond a cosine's size"
    assert bool(torch.isfinite(text).all()) and torch.allclose(text.norm(dim=-1), torch.ones(nl), atol=1e-6)


@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
@pytest.mark.parametrize("sc", SCENES, ids=_id)
def test_oracle_is_the_statement_and_obeys_the_rule(oracle, sc, mode):
    n, d, nl, dt, row0 = sc
    _, bad, text, is_bad = R.scene(n, d, nl, dt, row0)
    bad_np = is_bad.numpy()
    for epi, scale in R.EPILOGUES:
        if row0 and (epi != _abi.SAF_Q_SURGERY or mode != _abi.SAF_NORM_L2):
            continue  # (a bad row 0 matters to surgery alone, and only SAF_NORM_L2 makes it the zero row)
        what = f"{_id(sc)}, epilogue {epi}, mode {R.MODE_NAMES[mode]}"
        got = R.truth(oracle, n, d, nl, dt, row0, epi, scale, mode)
        with np.errstate(all="ignore"):
            want = R.statement(bad.float(), text, epi, scale, mode).numpy()
        # ---- the oracle is the statement
        g, w = got[~bad_np].astype(np.float64), want[~bad_np]
        assert np.isfinite(g).all() and np.isfinite(w).all(), f"{what}: a good row is not finite"
        err = np.abs(g - w)
        print(f"{what}: oracle against the float64 statement, good rows: max abs err {err.max():.3g}, "
              f"max err / (atol + rtol |want|) {(err / (HOST_ATOL + HOST_RTOL * np.abs(w))).max():.3g}")
        np.testing.assert_allclose(g, w, rtol=HOST_RTOL, atol=HOST_ATOL, err_msg=what)
        gb, wb = got[bad_np].astype(np.float64), want[bad_np]
        assert np.array_equal(np.isfinite(gb), np.isfinite(wb)), f"{what}: oracle and statement disagree on where a bad row is finite"
        both_inf = np.isinf(gb) & np.isinf(wb)
        assert np.array_equal(np.sign(gb[both_inf]), np.sign(wb[both_inf])), f"{what}: infinities of opposite sign"
        # ---- the oracle obeys the rule
        if mode == _abi.SAF_NORM_L2:
            zero = np.float32(R.zero_row(nl, epi))
            assert (got[bad_np] == zero).all(), f"{what}: a bad row is not the zero row ({zero} in every column)"
            assert (want[bad_np] == R.zero_row(nl, epi)).all(), f"{what}: the statement's bad rows"
        else:
            assert not np.isfinite(got[bad_np]).any(), f"{what}: a bad row has a finite output without nan_to_num"


@pytest.mark.parametrize("sc", [s for s in SCENES if s[4]], ids=_id)
def test_bad_row_zero_gives_uniform_surgery_weights(oracle, sc):
    """under SAF_NORM_L2 a bad row 0 is the zero row for the weights too: the surgery of the volume with the bad row 0 is the surgery
    of the volume whose row 0 is all zero, and that is S - mean_l S (every weight 1)"""
    n, d, nl, dt, _ = sc
    good, bad, text, is_bad = R.scene(n, d, nl, dt, True)
    got = R.truth(oracle, n, d, nl, dt, True, _abi.SAF_Q_SURGERY, 1.0, _abi.SAF_NORM_L2)
    zero0 = oracle.query_scan(good.float(), text, _abi.SAF_Q_SURGERY, scale=1.0, normalize=_abi.SAF_NORM_L2).numpy()
    keep = ~is_bad.numpy()
    assert np.array_equal(got[keep], zero0[keep])
    s = oracle.query_scan(good.float(), text, _abi.SAF_Q_SCORES, scale=1.0, normalize=_abi.SAF_NORM_L2).numpy().astype(np.float64)
    np.testing.assert_allclose(got[keep], (s - s.mean(axis=1, keepdims=True))[keep], rtol=HOST_RTOL, atol=HOST_ATOL)


@pytest.mark.parametrize("case", R.ROUTES + R.ONE_PER_ROUTE, ids=R.route_id)
def test_route_names_follow_the_dispatch_conditions(case):
    """the kernels the documented conditions give for a case are those its route is named after"""
    route, d, nl, dt, padded, env = case
    stride = d + 8 if padded else d
    R.check_route(route, R.expected_kernels(dt, stride, d, nl, _abi.SAF_Q_SOFTMAX, True, split_env=env))
    only_last = R.expected_kernels(dt, stride, d, nl, _abi.SAF_Q_SOFTMAX, False, split_env=env)
    assert only_last == (["query_kernel"] if route.startswith("blocks") or route == "wave-per-row" else [only_last[0]] * 1)
    assert R.expected_kernels(dt, stride, d, nl, _abi.SAF_Q_SURGERY, True, split_env=env)[0] == "query_kernel"


@pytest.mark.parametrize("case", R.TOPK_ROUTES, ids=R.route_id)
def test_topk_route_names_follow_the_dispatch_conditions(case):
    route, d, nl, dt = case
    R.check_route(route, R.expected_topk_kernels(dt, d, d, nl))


def test_stable_topk_prefers_the_smaller_label():
    s = torch.tensor([[0.0, 2.0, 2.0, -1.0, 2.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    assert R.stable_topk(s, 4).tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]]
