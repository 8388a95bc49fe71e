"""GPU: the small device passes of csrc/saf_misc.hip -- label argmax, sums <-> means, vertex sampling, the unwritten-row clear,
the lattice back-projection -- against their NumPy statements (tests/small_pass_reference.py), at the sizes where each kernel
takes another branch: the scalar and the 16-byte scaling kernel, ranges that do not start at voxel 0, rows of weight 0 that hold
data, the grid-stride loops past the launch cap (device CUs x 8 workgroups of 4 waves), ties and extreme counts in the argmax key,
corners and nearest voxels outside the volume, the 2-, 4- and 16-byte stores of the clear, every kind of invalid depth.

Exact passes are compared bit for bit; the trilinear blend and the back-projected points within 2^-20 of the statement's
magnitude (small_pass_reference.ERR_BOUND, derived there).  tests/test_small_passes_host.py holds the CPU oracle to the same
statements and bounds first, and checks that the planted inputs reach what they are planted for.  Each test prints its worst
err / bound (DESIGN.md quotes them).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import small_pass_reference as sp
from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd._lib import check, current_stream_ptr, lib

pytestmark = pytest.mark.gpu

_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(scope="module")
def cap_waves():
    """Waves of a wave-per-row kernel's largest grid: CUs x 8 workgroups x 4 waves (8192 on an MI355X)."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4


def _fusion(nvox, dim, dt=torch.float32):
    from spatially_aware_ai_amd import ClipFusion

    class FakeClip:
        feature_dim = dim

    return ClipFusion(torch.zeros(3), 0.1, torch.tensor(nvox), 0.3, False, FakeClip(), None, 10, 10, keep_xyz_world=False,
                      feat_dtype=dt).cuda()


# ---------------------------------------------------------------------------------------------- label argmax
def _argmax(lab):
    from spatially_aware_ai_amd.clip_seem_fusion import argmax_with_check

    out = argmax_with_check(torch.from_numpy(lab).cuda())
    assert out.dtype == torch.int64
    return out.cpu().numpy()


@pytest.mark.parametrize("n_classes", sp.ARGMAX_CLASSES)
def test_argmax_planted_rows(n_classes):
    rows, answer, names = sp.argmax_planted(n_classes)
    got = _argmax(rows)
    for k, name in enumerate(names):
        assert got[k] == answer[k], f"C = {n_classes}, row '{name}': {got[k]} instead of {answer[k]}"
    assert np.array_equal(_argmax(rows.astype(np.int64)), answer), "int64 histogram"
    # the same rows again and again, so that every lane position of a workgroup meets every row
    many = np.tile(rows, (5, 1))[: 4 * len(rows) + 3]
    assert np.array_equal(_argmax(many), np.tile(answer, 5)[: len(many)])


@pytest.mark.parametrize("n_classes", sp.ARGMAX_CLASSES)
@pytest.mark.parametrize("n_vox", [1, 3])
def test_argmax_few_rows(n_vox, n_classes):
    lab = sp.argmax_random(n_vox, n_classes, seed=n_vox + n_classes)
    assert np.array_equal(_argmax(lab), sp.label_argmax(lab))
    assert np.array_equal(_argmax(lab.astype(np.int64)), sp.label_argmax(lab))


@pytest.mark.parametrize("n_classes", [2, 65])
def test_argmax_past_the_launch_cap(cap_waves, n_classes):
    n_vox = 4 * cap_waves + 5
    lab = sp.argmax_random(n_vox, n_classes, seed=n_vox + n_classes)
    rows, answer, _ = sp.argmax_planted(n_classes)
    lab[-len(rows):] = rows  # the planted rows where only the stride loop reaches them
    want = sp.label_argmax(lab)
    assert np.array_equal(want[-len(rows):], answer)
    got = _argmax(lab)
    assert np.array_equal(got, want), f"{int((got != want).sum())} rows differ, the first at {int(np.nonzero(got != want)[0][0])}"


# ---------------------------------------------------------------------------------------------- sums <-> means
def _load(fusion, inp):
    fusion.clip_feat.copy_(torch.from_numpy(inp["feat"]))
    fusion.rgb.copy_(torch.from_numpy(inp["rgb"]))
    fusion.tsdf.copy_(torch.from_numpy(inp["tsdf"]))
    fusion.weight.copy_(torch.from_numpy(inp["weight"]))
    fusion.tsdf_weight.copy_(torch.from_numpy(inp["tsdf_weight"]))


def _scale_on_device(fusion, first, count, to_mean):
    from spatially_aware_ai_amd import distributed as dist

    if to_mean:
        dist.finalize_sums(fusion, first, count)
    else:  # (dist.means_to_sums always takes the whole volume)
        vol = fusion._c_volume()
        check(lib().saf_mean_to_sum(C.byref(vol), first, count, current_stream_ptr()), "saf_mean_to_sum")
    return fusion.clip_feat.cpu().numpy(), fusion.rgb.cpu().numpy(), fusion.tsdf.cpu().numpy()


def _check_scaled(got, inp, first, count, to_mean, what):
    want = sp.scale(inp["feat"], inp["rgb"], inp["tsdf"], inp["weight"], inp["tsdf_weight"], first, count, to_mean)
    n = len(inp["tsdf"])
    outside = np.ones(n, dtype=bool)
    outside[first:first + count] = False
    for g, w, orig, wname, name in zip(got, want, (inp["feat"], inp["rgb"], inp["tsdf"]), ("weight", "weight", "tsdf_weight"),
                                       ("clip_feat", "rgb", "tsdf")):
        assert sp.same_bits(g, w), f"{what}: {name} differs from the statement"
        assert g[outside].tobytes() == orig[outside].tobytes(), f"{what}: {name} changed outside the range"
        if to_mean:
            z = inp[wname] == 0
            assert g[z].tobytes() == orig[z].tobytes(), f"{what}: {name} changed in rows of weight 0"


@pytest.mark.parametrize("dim", sp.SCALE_DIMS)
@pytest.mark.parametrize("to_mean", [True, False])
def test_scaling_ranges(dim, to_mean):
    n = sp.N_GRID
    fusion = _fusion(sp.GRID, dim)
    inp = sp.scale_inputs(n, dim, seed=dim)
    for first, count in sp.scale_ranges(n):
        _load(fusion, inp)
        got = _scale_on_device(fusion, first, count, to_mean)
        _check_scaled(got, inp, first, count, to_mean, f"D = {dim}, voxels [{first}, {first + count}), to_mean = {to_mean}")


@pytest.mark.parametrize("to_mean", [True, False])
def test_scaling_past_the_launch_cap(cap_waves, to_mean):
    """D = 516 (16-byte accesses) over more voxels than the capped grid covers at once: count * D / 4 > cap * 256."""
    cap = cap_waves // 4
    dim, n = 516, cap * 2 + 3
    assert (n - 2) * (dim // 4) > cap * 256
    fusion = _fusion((n, 1, 1), dim)
    inp = sp.scale_inputs(n, dim, seed=dim)
    for first, count in ((0, n), (1, n - 2)):
        _load(fusion, inp)
        got = _scale_on_device(fusion, first, count, to_mean)
        _check_scaled(got, inp, first, count, to_mean, f"D = {dim}, voxels [{first}, {first + count}), to_mean = {to_mean}")


@pytest.mark.parametrize("dim", [6, 512])
def test_mean_to_sum_and_back_is_within_one_ulp(dim):
    n = sp.N_GRID
    fusion = _fusion(sp.GRID, dim)
    inp = sp.scale_inputs(n, dim, seed=dim)
    _load(fusion, inp)
    sums = _scale_on_device(fusion, 0, n, False)
    _check_scaled(sums, inp, 0, n, False, "means -> sums")
    got = _scale_on_device(fusion, 0, n, True)
    w, wt = inp["weight"], inp["tsdf_weight"]
    back = sp.scale(*sp.scale(inp["feat"], inp["rgb"], inp["tsdf"], w, wt, 0, n, False), w, wt, 0, n, True)
    for g, b, orig, mask, name in zip(got, back, (inp["feat"], inp["rgb"], inp["tsdf"]), (w > 0, w > 0, wt > 0), ("clip_feat", "rgb", "tsdf")):
        assert sp.same_bits(g, b), name
        ulps = np.abs(g[mask].astype(np.float64) - orig[mask]) / np.spacing(np.abs(orig[mask])).astype(np.float64)
        print(f"D = {dim}, {name}: mean -> sum -> mean moves a value by at most {ulps.max():.0f} ulp")
        assert ulps.max() <= 1.0
    # what saf_mean_to_sum leaves in a row of weight 0 (include/saf.h): x * 0 -- zero for finite data, NaN for NaN and inf
    z = w == 0
    f = sums[0][z]
    assert (f[np.isfinite(inp["feat"][z])] == 0).all() and np.isnan(f[~np.isfinite(inp["feat"][z])]).all()


# ---------------------------------------------------------------------------------------------- vertex sampling
@pytest.mark.parametrize("dim", sp.SAMPLE_DIMS)
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_vertex_sampling(cap_waves, dim, dt):
    v = sp.sample_volume(dim)
    verts, n_planted = sp.sample_vertex_set(max(0, cap_waves - 13 ** 3 - 500) + 37)
    assert len(verts) > cap_waves, "the vertices do not reach the grid-stride loop"
    fusion = _fusion(sp.GRID, dim, _DT[dt])
    feat = torch.from_numpy(v["feat"]).to(_DT[dt])  # rounded once, here; the kernel and the statement widen it exactly
    fusion.clip_feat.copy_(feat)
    fusion.rgb.copy_(torch.from_numpy(v["rgb"]))
    want = sp.sample_vertices(feat, v["rgb"], sp.GRID, verts, v["obj_idx"], v["seg_color"])
    bf, br = sp.ERR_BOUND * want["feat_mag"], sp.ERR_BOUND * want["rgb_mag"]
    first = None
    for extras in (True, False):
        out = fusion.sample_mesh_vertices(verts, *((v["obj_idx"], v["seg_color"]) if extras else ()))
        assert len(out) == (4 if extras else 2)
        rgb, got = (t.cpu().numpy() for t in out[:2])
        ef = np.abs(got.astype(np.float64) - want["feat"])
        er = np.abs(rgb.astype(np.float64) - np.clip(want["rgb"], 0, 1))
        print(f"D = {dim}, {dt}, obj / seg {'given' if extras else 'absent'}: worst err / bound: features "
              f"{(ef[bf > 0] / bf[bf > 0]).max():.3f}, rgb {(er[br > 0] / br[br > 0]).max():.3f}")
        bad = np.nonzero((ef > bf).any(axis=1))[0]
        assert len(bad) == 0, f"features of {len(bad)} vertices off, the first: vertex {bad[0]} at {verts[bad[0]]}"
        bad = np.nonzero((er > br).any(axis=1))[0]
        assert len(bad) == 0, f"rgb of {len(bad)} vertices off, the first: vertex {bad[0]} at {verts[bad[0]]}"
        assert rgb.min() == 0.0 and rgb.max() == 1.0, "the clamp"
        if extras:
            obj, seg = out[2].cpu().numpy(), out[3].cpu().numpy()
            assert obj.shape == (len(verts), 1) and np.array_equal(obj[:, 0], want["obj"]), "nearest object index"
            assert np.array_equal(seg, want["seg"]), "nearest segmentation colour"
            first = (rgb, got)
        else:
            assert np.array_equal(rgb, first[0]) and np.array_equal(got, first[1]), "obj / seg change the blend"


# ---------------------------------------------------------------------------------------------- unwritten-row clear
def _clear_on_device(fusion, data, weight, first, rows):
    raw = fusion.clip_feat.view(torch.uint8)
    assert tuple(raw.shape) == data.shape
    raw.copy_(torch.from_numpy(data))
    fusion.weight.copy_(torch.from_numpy(weight))
    vol = fusion._c_volume()
    check(lib().saf_clear_unwritten_rows(C.byref(vol), first, rows, current_stream_ptr()), "saf_clear_unwritten_rows")
    return fusion.clip_feat.view(torch.uint8).cpu().numpy()


def _assert_cleared(got, data, weight, first, rows, what):
    want = sp.clear_unwritten(data, weight, first, rows)
    if not np.array_equal(got, want):
        r = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(r)} rows differ, the first: row {r[0]} (weight {weight[r[0]]}), bytes "
                             f"{np.nonzero(got[r[0]] != want[r[0]])[0][:8]}")


@pytest.mark.parametrize("dt,dim", sp.CLEAR_SHAPES)
def test_clear_row_sizes_and_ranges(dt, dim):
    n = sp.N_GRID
    fusion = _fusion(sp.GRID, dim, _DT[dt])
    rb = dim * fusion.clip_feat.element_size()
    data, weight = sp.clear_inputs(n, rb, seed=rb)
    for first, rows in sp.clear_ranges(n):
        got = _clear_on_device(fusion, data, weight, first, rows)
        _assert_cleared(got, data, weight, first, rows, f"{dt}, D = {dim} ({rb} bytes), rows [{first}, {first + rows})")


def test_clear_past_the_launch_cap(cap_waves, monkeypatch):
    """One workgroup per CU (SAF_CLEAR_WGS=1, read per call) over 256 x CUs + 77 rows: the last rows belong to the stride loop."""
    monkeypatch.setenv("SAF_CLEAR_WGS", "1")
    n = 256 * (cap_waves // 32) + 77
    fusion = _fusion((n, 1, 1), 8, torch.float16)
    data, weight = sp.clear_inputs(n, 16, seed=3)
    assert (weight[-77:] == 0).sum() > 20
    for first, rows in ((0, n), (1, n - 2)):
        got = _clear_on_device(fusion, data, weight, first, rows)
        _assert_cleared(got, data, weight, first, rows, f"rows [{first}, {first + rows})")


# ---------------------------------------------------------------------------------------------- lattice back-projection
def test_backproject_lattices_and_invalid_depths():
    pose, kinv = sp.backproject_camera()
    pose_d, kinv_d = torch.from_numpy(pose).cuda(), torch.from_numpy(kinv).cuda()
    worst = 0.0
    for name, depth, u, v, hit in sp.backproject_cases():
        want, valid, mag = sp.backproject(depth, pose, kinv, u, v, sp.MAX_DEPTH)
        m = len(u) * len(v)
        depth_d, u_d, v_d = torch.from_numpy(depth).cuda(), torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
        xyz = torch.full((m + 1, 3), 77.0, dtype=torch.float32, device="cuda")
        got_valid = torch.full((m + 1,), 7, dtype=torch.uint8, device="cuda")
        rc = lib().saf_backproject_lattice(depth_d.data_ptr(), depth.shape[0], depth.shape[1], pose_d.data_ptr(), kinv_d.data_ptr(),
                                           u_d.data_ptr(), len(u), v_d.data_ptr(), len(v), float(sp.MAX_DEPTH), xyz.data_ptr(),
                                           got_valid.data_ptr(), current_stream_ptr())
        check(rc, "saf_backproject_lattice")
        xyz, got_valid = xyz.cpu().numpy(), got_valid.cpu().numpy()
        assert got_valid[m] == 7 and (xyz[m] == 77.0).all(), f"{name}: wrote past the lattice"
        for s, o in hit.items():
            assert bool(got_valid[o]) == sp.SPECIAL_VALID[s], f"{name}: depth '{s}' is reported {'valid' if got_valid[o] else 'invalid'}"
        assert np.array_equal(got_valid[:m], valid.astype(np.uint8)), name
        fin = np.isfinite(depth[np.repeat(v, len(u)), np.tile(u, len(v))])
        with np.errstate(invalid="ignore"):
            err, bound = np.abs(xyz[:m].astype(np.float64) - want)[fin], sp.ERR_BOUND * mag[fin]
        assert (err <= bound).all(), f"{name}: point {int(np.nonzero((err > bound).any(axis=1))[0][0])} of the finite ones is off"
        worst = max(worst, float((err / bound).max()))
    print(f"back-projection, worst err / bound: xyz {worst:.3f}")
