"""CPU: the NumPy statements of the small device passes (tests/small_pass_reference.py) against the CPU oracle, on the inputs
tests/test_small_passes_gpu.py gives the HIP kernels, and the host side of the six entry points.

  * label argmax, sums <-> means and `valid` of the back-projection: the oracle equals the statement bit for bit;
  * vertex sampling and the back-projected points: the oracle (fp32, the kernel's arithmetic) lies within 2^-20 of the
    magnitude of the float64 statement -- the bound the GPU tests assert; the worst err / bound is printed per pass;
  * the planted inputs are not hollow: enough vertices have a skipped corner, sample nearest outside the volume and clamp at
    both ends; every special depth is reached; every planted histogram row has the answer its name says;
  * saf_label_argmax, saf_merge_finalize, saf_mean_to_sum, saf_sample_vertices, saf_clear_unwritten_rows and
    saf_backproject_lattice refuse bad arguments, and accept empty work, on the host (no GPU needed: nothing is launched).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import small_pass_reference as sp
from host_stubs import P, fake_volume  # P: every call of the host-side tests below returns before it would be used
from spatially_aware_ai_amd import _abi, _lib

CUS = 256  # an MI355X; the GPU tests read the device's count
CAP_WAVES = CUS * 8 * 4


# ---------------------------------------------------------------------------------------------- label argmax
@pytest.mark.parametrize("n_classes", sp.ARGMAX_CLASSES)
def test_argmax_statement_on_the_planted_rows(oracle, n_classes):
    rows, answer, names = sp.argmax_planted(n_classes)
    got = sp.label_argmax(rows)
    for k, name in enumerate(names):
        assert got[k] == answer[k], f"C = {n_classes}, row '{name}': the statement says {got[k]}, the row was made for {answer[k]}"
    assert np.array_equal(oracle.label_argmax(rows).numpy(), answer), "the oracle disagrees on a planted row"
    if n_classes >= 65:
        assert {"tie at (63, 64)", "tie at (0, 64)", "maximum only in the last partial group"} <= set(names)


@pytest.mark.parametrize("n_vox,n_classes", [(n, c) for c in sp.ARGMAX_CLASSES for n in (1, 3)] + [(4 * CAP_WAVES + 5, 2),
                                                                                                   (4 * CAP_WAVES + 5, 65)])
def test_argmax_statement_against_the_oracle(oracle, n_vox, n_classes):
    lab = sp.argmax_random(n_vox, n_classes, seed=n_vox + n_classes)
    want = sp.label_argmax(lab)
    assert np.array_equal(oracle.label_argmax(lab).numpy(), want)
    if n_vox > 100:
        assert (want == -1).mean() > 0.2 and (want > 0).any() and (lab < 0).any(), "the random rows lost a kind"


# ---------------------------------------------------------------------------------------------- sums <-> means
def _oracle_scale(oracle, inp, dim, first, count, to_mean):
    n = len(inp["tsdf"])
    vol = oracle.OracleVolume(torch.zeros(3), 0.1, (n, 1, 1), 0.3, dim)
    vol.clip_feat, vol.rgb, vol.tsdf = (torch.from_numpy(inp[k].copy()) for k in ("feat", "rgb", "tsdf"))
    vol.weight, vol.tsdf_weight = torch.from_numpy(inp["weight"].copy()), torch.from_numpy(inp["tsdf_weight"].copy())
    fn = oracle.lib().saf_oracle_merge_finalize if to_mean else oracle.lib().saf_oracle_mean_to_sum
    assert fn(C.byref(vol.c_volume()), first, count) == 0
    return vol.clip_feat.numpy(), vol.rgb.numpy(), vol.tsdf.numpy()


@pytest.mark.parametrize("dim", sp.SCALE_DIMS)
@pytest.mark.parametrize("to_mean", [True, False])
def test_scale_statement_against_the_oracle(oracle, dim, to_mean):
    n = sp.N_GRID
    inp = sp.scale_inputs(n, dim, seed=dim)
    for first, count in sp.scale_ranges(n):
        want = sp.scale(inp["feat"], inp["rgb"], inp["tsdf"], inp["weight"], inp["tsdf_weight"], first, count, to_mean)
        got = _oracle_scale(oracle, inp, dim, first, count, to_mean)
        for g, w, name in zip(got, want, ("clip_feat", "rgb", "tsdf")):
            assert sp.same_bits(g, w), f"{name}, voxels [{first}, {first + count}), to_mean = {to_mean}"


def test_scale_inputs_are_not_hollow():
    n = sp.N_GRID
    for dim in sp.SCALE_DIMS:
        inp = sp.scale_inputs(n, dim, seed=dim)
        w, wt = inp["weight"], inp["tsdf_weight"]
        assert set(np.unique(w)) == set(sp.SCALE_WEIGHTS) == set(np.unique(wt))
        assert ((w == 0) & (wt > 0)).sum() >= 10 and ((w > 0) & (wt == 0)).sum() >= 10, "one weight zero, the other not"
        z = w == 0
        assert np.isnan(inp["feat"][z]).any() and np.isinf(inp["feat"][z]).any() and np.isfinite(inp["feat"][z]).all(axis=1).any()
        assert np.isfinite(inp["feat"][~z]).all() and (inp["feat"][np.isfinite(inp["feat"])] != 0).all()
        assert np.isnan(inp["tsdf"][wt == 0]).any() and np.isinf(inp["tsdf"][wt == 0]).any()
        # to_mean leaves the rows of weight 0 alone, whatever they hold; a range leaves every voxel outside it alone
        first, count = 1, n - 2
        f, r, t = sp.scale(inp["feat"], inp["rgb"], inp["tsdf"], w, wt, first, count, True)
        assert f[z].tobytes() == inp["feat"][z].tobytes() and r[z].tobytes() == inp["rgb"][z].tobytes()
        assert t[wt == 0].tobytes() == inp["tsdf"][wt == 0].tobytes()
        for a, b in ((f, inp["feat"]), (r, inp["rgb"]), (t, inp["tsdf"])):
            assert a[0].tobytes() == b[0].tobytes() and a[-1].tobytes() == b[-1].tobytes()
            assert not sp.same_bits(a[1], b[1]) and not sp.same_bits(a[n - 2], b[n - 2]), "the range's end voxels are scaled"
        # 2^24 + 1 is not a float32: the kernel's (float)w rounds it, and so must the statement
        k = np.nonzero(w == 2 ** 24 + 1)[0][0]
        assert f[k, 1] == inp["feat"][k, 1] / np.float32(2 ** 24)


def test_round_trip_is_within_one_ulp():
    """mean -> sum -> mean: two roundings, at most one unit in the last place of the original (where w > 0)."""
    n, dim = sp.N_GRID, 7
    inp = sp.scale_inputs(n, dim, seed=dim)
    w, wt = inp["weight"], inp["tsdf_weight"]
    s = sp.scale(inp["feat"], inp["rgb"], inp["tsdf"], w, wt, 0, n, False)
    m = sp.scale(*s, w, wt, 0, n, True)
    for got, orig, mask in ((m[0], inp["feat"], w > 0), (m[1], inp["rgb"], w > 0), (m[2], inp["tsdf"], wt > 0)):
        ulps = np.abs(got[mask].astype(np.float64) - orig[mask]) / np.spacing(np.abs(orig[mask])).astype(np.float64)
        assert ulps.max() <= 1.0 and ulps.max() > 0, ulps.max()


# ---------------------------------------------------------------------------------------------- vertex sampling
def _extra():
    return CAP_WAVES - 13 ** 3 - 500 + 37


@pytest.mark.parametrize("dim", sp.SAMPLE_DIMS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])  # (the oracle has no fp16 volume)
def test_sampling_oracle_within_the_bound_of_the_statement(oracle, dim, dt):
    v = sp.sample_volume(dim)
    verts, n_planted = sp.sample_vertex_set(_extra())
    assert len(verts) > CAP_WAVES
    feat = torch.from_numpy(v["feat"]).to(dt)
    vol = oracle.OracleVolume(torch.zeros(3), 0.1, sp.GRID, 0.3, dim, feat_dtype=dt)
    vol.clip_feat, vol.rgb = feat, torch.from_numpy(v["rgb"])
    for extras in (True, False):
        oi, sc = (v["obj_idx"], v["seg_color"]) if extras else (None, None)
        want = sp.sample_vertices(feat, v["rgb"], sp.GRID, verts, oi, sc)
        gf, gr, go, gs = oracle.sample_vertices(vol, verts, oi, sc)
        ef = np.abs(gf.double().numpy() - want["feat"])
        er = np.abs(gr.double().numpy() - np.clip(want["rgb"], 0, 1))
        bf, br = sp.ERR_BOUND * want["feat_mag"], sp.ERR_BOUND * want["rgb_mag"]
        print(f"D = {dim}, {dt}: oracle vs statement, worst err / bound: features {(ef[bf > 0] / bf[bf > 0]).max():.3f}, "
              f"rgb {(er[br > 0] / br[br > 0]).max():.3f}")
        assert (ef <= bf).all() and (er <= br).all()
        if extras:
            assert np.array_equal(go.numpy(), want["obj"]) and np.array_equal(gs.numpy(), want["seg"])
        else:
            assert go is None and gs is None and want["obj"] is None and want["seg"] is None


def test_sampling_inputs_are_not_hollow():
    verts, n_planted = sp.sample_vertex_set(0)
    assert n_planted == 13 ** 3 and len(verts) == n_planted + 500
    for dim in sp.SAMPLE_DIMS:
        v = sp.sample_volume(dim)
        want = sp.sample_vertices(v["feat"], v["rgb"], sp.GRID, verts, v["obj_idx"], v["seg_color"])
        skipped, out = want["skipped"][:n_planted].mean(), want["nearest_out"][:n_planted].mean()
        print(f"D = {dim}: {skipped:.1%} of the planted vertices skip a corner, {out:.1%} sample nearest outside the volume")
        assert skipped >= 0.30 and out >= 0.10
        assert not want["skipped"][n_planted:].any() and not want["nearest_out"][n_planted:].any(), "the interior vertices"
        assert (want["rgb"] < 0).sum() > 20 and (want["rgb"] > 1).sum() > 20, "both ends of the rgb clamp"
        inside = ~want["nearest_out"]
        assert (want["seg"][inside] == 0).any() and (want["seg"][inside] == 1).any() and (want["obj"] < 0).any()
        assert (want["obj"][want["nearest_out"]] == 0).all() and (want["seg"][want["nearest_out"]] == 0).all()
    # a swap of two axes is visible: the vertex (0, 0, nz - 1) is in the volume along z only
    one = sp.sample_vertices(v["feat"], v["rgb"], sp.GRID, np.array([[0, 0, sp.GRID[2] - 1]], dtype=np.float32))
    assert np.array_equal(one["feat"][0], v["feat"][sp.GRID[2] - 1].astype(np.float64))
    # a vertex on a voxel takes that voxel's row exactly; half-way between two voxels the mean of the two rows
    mid = sp.sample_vertices(v["feat"], v["rgb"], sp.GRID, np.array([[1.5, 2, 3]], dtype=np.float32))
    r0, r1 = ((x * 7 + 2) * 9 + 3 for x in (1, 2))
    assert np.allclose(mid["feat"][0], (v["feat"][r0].astype(np.float64) + v["feat"][r1]) / 2, rtol=1e-6, atol=1e-4)


# ---------------------------------------------------------------------------------------------- lattice back-projection
def test_backprojection_oracle_within_the_bound_of_the_statement(oracle):
    pose, kinv = sp.backproject_camera()
    reached = set()
    worst = 0.0
    for name, depth, u, v, hit in sp.backproject_cases():
        want, valid, mag = sp.backproject(depth, pose, kinv, u, v, sp.MAX_DEPTH)
        xyz, got_valid = oracle.backproject_lattice(depth, pose, kinv, u, v, float(sp.MAX_DEPTH))
        assert np.array_equal(got_valid.numpy(), valid), name
        for s, o in hit.items():
            assert valid[o] == sp.SPECIAL_VALID[s], f"{name}: depth '{s}'"
        reached |= set(hit)
        d = depth[np.repeat(v, len(u)), np.tile(u, len(v))]
        fin = np.isfinite(d)
        with np.errstate(invalid="ignore"):  # (inf - inf at the non-finite depths, which are masked out)
            err, bound = np.abs(xyz.double().numpy() - want)[fin], sp.ERR_BOUND * mag[fin]
        assert (err <= bound).all(), name
        worst = max(worst, float((err / bound).max()))
        assert 0.2 < valid.mean() < 0.95 or len(valid) < 10, name
    print(f"oracle vs statement, worst err / bound: xyz {worst:.3f}")
    assert reached == set(sp.SPECIAL_DEPTHS)
    name, depth, u, v, hit = sp.backproject_cases()[0]
    assert set(hit) == set(sp.SPECIAL_DEPTHS), "the full grid reaches every special depth"
    name, depth, u, v, hit = sp.backproject_cases()[-1]
    assert len(u) * len(v) > 256 and (len(u) * len(v)) % 256 and set(hit) == set(sp.SPECIAL_DEPTHS)
    assert hit["nan"] == len(u) * len(v) - 1


# ---------------------------------------------------------------------------------------------- unwritten-row clear
def test_clear_inputs_are_not_hollow():
    n = sp.N_GRID
    for dt, dim in sp.CLEAR_SHAPES:
        rb = dim * (4 if dt == "f32" else 2)
        data, weight = sp.clear_inputs(n, rb, seed=rb)
        assert (data != 0).all() and 0.4 < (weight == 0).mean() < 0.7 and weight[0] == 0 and weight[n - 1] == 0
        z = np.concatenate([[1], weight != 0, [1]])
        runs = np.diff(np.nonzero(z)[0]) - 1
        assert runs.max() >= 64
        for first, rows in sp.clear_ranges(n):
            out = sp.clear_unwritten(data, weight, first, rows)
            inside = np.zeros(n, dtype=bool)
            inside[first:first + rows] = True
            cleared = inside & (weight == 0)
            assert cleared.any() and (out[cleared] == 0).all() and np.array_equal(out[~cleared], data[~cleared])
            if first > 0:
                assert weight[first - 1] == 0 and weight[first + rows] == 0, "unwritten rows right outside the range are kept"
    assert sorted({d * (4 if t == "f32" else 2) for t, d in sp.CLEAR_SHAPES}) == [10, 12, 16, 32, 48, 72]


# ---------------------------------------------------------------------------------------------- the host side of the entry points
def _fake_volume(**fields):
    return C.byref(fake_volume(n=4, dim=8, **fields))


@pytest.mark.parametrize("fn", ["saf_merge_finalize", "saf_mean_to_sum"])
def test_scaling_rejects_bad_arguments_on_the_host(fn):
    call = getattr(_lib.lib(), fn)
    n = 64
    for vol, first, count in [(None, 0, 1), (_fake_volume(clip_feat=None), 0, 1), (_fake_volume(weight=None), 0, 1),
                              (_fake_volume(tsdf_weight=None), 0, 1), (_fake_volume(rgb=None), 0, 1), (_fake_volume(tsdf=None), 0, 1),
                              (_fake_volume(), -1, 1), (_fake_volume(), 0, -1), (_fake_volume(), 0, n + 1), (_fake_volume(), n, 1),
                              (_fake_volume(), 60, 5)]:
        assert call(vol, first, count, None) == _abi.SAF_E_INVALID, (first, count)
        assert b"merge" in _lib.lib().saf_last_error()
    for dt in (_abi.SAF_BF16, _abi.SAF_F16):
        assert call(_fake_volume(dtype=dt), 0, 1, None) == _abi.SAF_E_UNSUPPORTED
    for first in (0, 7, n):
        assert call(_fake_volume(), first, 0, None) == _abi.SAF_OK


def test_label_argmax_rejects_bad_arguments_on_the_host():
    call = _lib.lib().saf_label_argmax
    for lab, n, c, out in [(None, 1, 1, P), (P, 1, 1, None), (P, -1, 1, P), (P, 1, 0, P), (P, 1, -3, P)]:
        assert call(lab, n, c, out, None) == _abi.SAF_E_INVALID, (lab, n, c, out)
        assert b"label_argmax" in _lib.lib().saf_last_error()
    assert call(P, 0, 143, P, None) == _abi.SAF_OK


def test_sample_vertices_rejects_bad_arguments_on_the_host():
    call = _lib.lib().saf_sample_vertices
    good = dict(vol=_fake_volume(), verts=P, n=1, feat=P, rgb=P, oi=None, oo=None, sc=None, so=None)
    bad = [dict(vol=None), dict(vol=_fake_volume(clip_feat=None)), dict(vol=_fake_volume(rgb=None)), dict(verts=None), dict(feat=None),
           dict(rgb=None), dict(n=-1), dict(oi=P), dict(sc=P), dict(oi=P, oo=P, sc=P), dict(oi=P, sc=P, so=P)]
    for change in bad:
        a = dict(good, **change)
        rc = call(a["vol"], a["verts"], a["n"], a["feat"], a["rgb"], a["oi"], a["oo"], a["sc"], a["so"], None)
        assert rc == _abi.SAF_E_INVALID, change
        assert b"sample_vertices" in _lib.lib().saf_last_error()
    assert call(_fake_volume(dtype=7), P, 1, P, P, None, None, None, None, None) == _abi.SAF_E_UNSUPPORTED
    for dt in (_abi.SAF_F32, _abi.SAF_BF16, _abi.SAF_F16):
        assert call(_fake_volume(dtype=dt), P, 0, P, P, P, P, P, P, None) == _abi.SAF_OK


def test_clear_rejects_bad_arguments_on_the_host():
    call = _lib.lib().saf_clear_unwritten_rows
    n = 64
    for vol, first, rows in [(None, 0, 1), (_fake_volume(clip_feat=None), 0, 1), (_fake_volume(weight=None), 0, 1), (_fake_volume(), -1, 1),
                             (_fake_volume(), 0, -1), (_fake_volume(), 0, n + 1), (_fake_volume(), n, 1),
                             (_fake_volume(clip_feat=P + 4), 0, 1), (_fake_volume(clip_feat=P + 8, dtype=_abi.SAF_F16), 3, 2)]:
        assert call(vol, first, rows, None) == _abi.SAF_E_INVALID, (first, rows)
        assert b"clear_unwritten_rows" in _lib.lib().saf_last_error()
    assert b"16-byte aligned" in _lib.lib().saf_last_error()
    assert call(_fake_volume(), 0, 0, None) == _abi.SAF_OK and call(_fake_volume(), n, 0, None) == _abi.SAF_OK


def test_backproject_rejects_bad_arguments_on_the_host():
    call = _lib.lib().saf_backproject_lattice
    good = dict(depth=P, h=7, w=9, pose=P, kinv=P, u=P, nu=3, v=P, nv=3, xyz=P, valid=P)
    bad = [dict(depth=None), dict(pose=None), dict(kinv=None), dict(u=None), dict(v=None), dict(xyz=None), dict(valid=None),
           dict(h=0), dict(w=-1), dict(nu=0), dict(nu=-2), dict(nv=0)]
    for change in bad:
        a = dict(good, **change)
        rc = call(a["depth"], a["h"], a["w"], a["pose"], a["kinv"], a["u"], a["nu"], a["v"], a["nv"], 3.0, a["xyz"], a["valid"], None)
        assert rc == _abi.SAF_E_INVALID, change
        assert b"backproject" in _lib.lib().saf_last_error()
