"""CPU: the host side of float16 fusion volumes (SAF_F16 as `saf_volume.feat_dtype`) -- the route and the workspace an fp16
descriptor gets (those of a bf16 descriptor on the widths the row kernels take, the per-frame pipeline elsewhere: the brick
form does not take fp16), the refusal of SAF_SUM, the module's constructor -- and the self-consistency of the stepped oracle that
tests/test_fp16_volume_gpu.py compares the device with (tests/fp16_reference.py).  No HIP call, no device pointer followed."""
import ctypes as C
import os

import pytest
import torch

from spatially_aware_ai_amd import _abi, _lib
from spatially_aware_ai_amd import synthetic as syn

import fp16_reference as ref

ADDR = 0x7F0000000000  # non-null, 256-byte aligned; the host-only entries never follow it
H, W, NPY, NPX = 480, 640, 30, 40
ROUTE_ENVS = [{}, {"SAF_WIN_FORM": "rows"}, {"SAF_WIN_FORM": "sums"}, {"SAF_WINDOW": "0"}, {"SAF_WINDOW_BF16": "0"},
              {"SAF_WIN_MAPS16": "0"}, {"SAF_WIN_FRAMES": "64"}, {"SAF_WIN_OVERLAP": "0"}]


def _volume(dim, dtype, grid=(61, 60, 59), accum=_abi.SAF_RUNNING_MEAN, n_classes=0):
    v = _abi.SafVolume()
    v.nx, v.ny, v.nz = grid
    v.feat_dim, v.n_classes, v.feat_dtype, v.accum_mode, v.trunc = dim, n_classes, dtype, accum, 0.1
    for name in ("axis_x", "axis_y", "axis_z", "tsdf", "tsdf_weight", "weight", "rgb", "clip_feat"):
        setattr(v, name, ADDR)
    v.labels_one_hot = ADDR if n_classes else None
    return v


def _frames(n):
    frames = (_abi.SafFrame * n)()
    for f in frames:
        f.height, f.width, f.npy, f.npx = H, W, NPY, NPX
        f.depth = f.rgb = f.pose = f.K = f.feat_map = ADDR
    return frames


def _answers(lib, dim, dtype, n_frames, **kw):
    """(bytes_for, bytes_for_frames, [path, session at both sizes and one byte below each])."""
    vol, frames = _volume(dim, dtype, **kw), _frames(n_frames)
    sizes = [int(lib.saf_fuse_workspace_bytes_for(C.byref(vol), NPY, NPX)),
             int(lib.saf_fuse_workspace_bytes_for_frames(C.byref(vol), NPY, NPX, H, W))]
    routes = [(lib.saf_fuse_path(C.byref(vol), frames, n_frames, ws), lib.saf_fuse_session_ok(C.byref(vol), frames, n_frames, ws))
              for b in sizes for ws in (b, max(b - 1, 0))]
    return sizes, routes


@pytest.mark.parametrize("env", ROUTE_ENVS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_fp16_descriptor_is_routed_and_sized_as_bf16_on_the_row_kernels_widths(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = _lib.lib()
    for dim in (512, 1024):
        for n_classes in (0, 7):
            h = _answers(lib, dim, _abi.SAF_F16, 16, n_classes=n_classes)
            b = _answers(lib, dim, _abi.SAF_BF16, 16, n_classes=n_classes)
            assert h == b, (dim, env, h, b)
            assert all(p in (0, 1) and s in (0, 1) for p, s in h[1]) and min(h[0]) > 0
    if not env:
        # SAF_WIN_FORM=bricks on these widths: the brick form does not take fp16 -- the call stays windowed (the default form),
        # a session still takes it, and no pools are reserved (a bf16 volume's workspace grows by them)
        monkeypatch.setenv("SAF_WIN_FORM", "bricks")
        asked, same16 = _answers(lib, 512, _abi.SAF_F16, 16), _answers(lib, 512, _abi.SAF_BF16, 16)
        monkeypatch.delenv("SAF_WIN_FORM")
        assert asked == _answers(lib, 512, _abi.SAF_F16, 16) and asked[1][0] == (1, 1) and same16[0][0] > asked[0][0]
    if not env:  # the default route of a 16-frame call is the windowed path
        vol, frames = _volume(512, _abi.SAF_F16), _frames(16)
        ws = lib.saf_fuse_workspace_bytes_for(C.byref(vol), NPY, NPX)
        assert lib.saf_fuse_path(C.byref(vol), frames, 16, ws) == 1 and lib.saf_fuse_session_ok(C.byref(vol), frames, 16, ws) == 1


@pytest.mark.parametrize("env", [{}, {"SAF_WIN_FORM": "bricks"}, {"SAF_WIN_FORM": "rows"}], ids=["default", "bricks", "rows"])
def test_fp16_widths_without_a_row_kernel_stay_on_the_per_frame_pipeline(env, monkeypatch):
    """The brick form takes f32 and bf16 rows only: where a bf16 volume of such a width goes to it, an fp16 volume's call takes the
    per-frame pipeline (0) -- never -1, the answer for a descriptor the library refuses (and the answer for every fp16 descriptor
    before fp16 fusion existed)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lib = _lib.lib()
    for dim in (64, 256, 768):
        sizes, routes = _answers(lib, dim, _abi.SAF_F16, 16)
        assert [p for p, _ in routes] == [0, 0, 0, 0], (dim, routes)
        assert min(sizes) > 0
    for dim in (8, 24, 64, 128, 256, 512, 768, 1024, 2048):  # any width a 16-bit volume may have
        for n in (1, 15, 16, 129):
            vol, frames = _volume(dim, _abi.SAF_F16), _frames(n)
            for ws in (0, 1 << 20, 1 << 40):
                assert lib.saf_fuse_path(C.byref(vol), frames, n, ws) in (0, 1), (dim, n, ws)
                assert lib.saf_fuse_session_ok(C.byref(vol), frames, n, ws) in (0, 1), (dim, n, ws)
    # an fp16 volume never reserves the brick form's pools: its workspace is what SAF_WIN_FORM=rows gives it
    sizes_env = _answers(lib, 64, _abi.SAF_F16, 16)[0]
    monkeypatch.setenv("SAF_WIN_FORM", "rows")
    assert _answers(lib, 64, _abi.SAF_F16, 16)[0] == sizes_env


def test_fp16_descriptor_conditions_are_the_bf16_ones():
    lib = _lib.lib()
    frames = _frames(16)
    for dim in (4, 12, 63):  # feat_dim % 8 != 0
        for dt in (_abi.SAF_F16, _abi.SAF_BF16):
            vol = _volume(dim, dt)
            assert lib.saf_fuse_path(C.byref(vol), frames, 16, 1 << 30) == -1
            assert lib.saf_fuse_workspace_bytes_for(C.byref(vol), NPY, NPX) == 0
    vol = _volume(64, _abi.SAF_F16)
    vol.clip_feat = ADDR + 8  # rows off the 16-byte boundary
    assert lib.saf_fuse_path(C.byref(vol), frames, 16, 1 << 30) == -1
    vol = _volume(64, 3)  # no such dtype
    assert lib.saf_fuse_path(C.byref(vol), frames, 16, 1 << 30) == -1


def test_sum_mode_into_an_fp16_volume_is_refused():
    lib = _lib.lib()
    vol, frames = _volume(512, _abi.SAF_F16, accum=_abi.SAF_SUM), _frames(16)
    assert lib.saf_fuse_path(C.byref(vol), frames, 16, 1 << 30) == -1
    assert lib.saf_fuse_session_ok(C.byref(vol), frames, 16, 1 << 30) == -1
    assert lib.saf_fuse_workspace_bytes_for(C.byref(vol), NPY, NPX) == 0
    # the fusion entries refuse the descriptor before anything touches the device
    rc = lib.saf_fuse_frames(C.byref(vol), frames, 16, ADDR, 1 << 30, None, None)
    assert rc == _abi.SAF_E_UNSUPPORTED
    msg = lib.saf_last_error().decode()
    assert "SAF_SUM" in msg and "fp16" in msg, msg
    for dt in (_abi.SAF_F32, _abi.SAF_BF16):  # the other dtypes keep their sums
        assert lib.saf_fuse_path(C.byref(_volume(512, dt, accum=_abi.SAF_SUM)), frames, 16, 1 << 30) in (0, 1)


class _Clip:
    feature_dim = 512

    def img_inference_tiled(self, rgb, patch_size, patch_stride):
        raise AssertionError("not called")


@pytest.mark.parametrize("seem", [False, True])
def test_modules_accept_float16(seem):
    from spatially_aware_ai_amd import ClipFusion, ClipSeemFusion

    grid = syn.make_grid((8, 6, 10))
    if seem:
        fz = ClipSeemFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, 10, 10, _Clip(), None,
                            keep_xyz_world=False, feat_dtype=torch.float16)
    else:
        fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, _Clip(), None, 10, 10,
                        keep_xyz_world=False, feat_dtype=torch.float16)
    feat = fz._buffers["clip_feat"]
    assert feat.dtype == torch.float16 and tuple(feat.shape) == (480, 512) and feat.element_size() == 2
    assert "clip_feat" in fz.state_dict() and fz.state_dict()["clip_feat"].dtype == torch.float16
    with pytest.raises(ValueError, match="feat_dtype"):
        ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, _Clip(), None, 10, 10, feat_dtype=torch.float64)
    # SAF_SUM is refused before a frame is queued
    fz.accum_mode = _abi.SAF_SUM
    z = torch.zeros
    with pytest.raises(_lib.SafError, match="SAF_SUM"):
        fz.integrate_features(z(1, 48, 64), z(1, 48, 64, 3), torch.eye(4)[None], torch.eye(3)[None], z(1, 512, 5, 7))


def test_frame_sharded_merge_refuses_an_fp16_volume_before_any_collective():
    from spatially_aware_ai_amd import ClipFusion
    from spatially_aware_ai_amd import distributed as D

    grid = syn.make_grid((8, 6, 10))
    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, _Clip(), None, 10, 10, keep_xyz_world=False,
                    feat_dtype=torch.float16)
    with pytest.raises(_lib.SafError, match="f32 feature volume"):
        D._require_f32_sums(fz, "merge_volumes")
    with pytest.raises(_lib.SafError, match="f32 feature volume"):
        D.fuse_merge_pipelined(fz, None, 0, None)


def test_shard_features_16_returns_the_rows_themselves():
    from spatially_aware_ai_amd import ClipFusion
    from spatially_aware_ai_amd import distributed as D

    grid = syn.make_grid((8, 6, 10))
    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, _Clip(), None, 10, 10, keep_xyz_world=False,
                    feat_dtype=torch.float16)
    whole = D.shard_features_16(fz, 0, 480, torch.float16)
    assert whole.data_ptr() == fz.clip_feat.data_ptr() and whole.dtype == torch.float16 and tuple(whole.shape) == (480, 512)
    part = D.shard_features_16(fz, 100, 50, torch.float16)
    assert part.data_ptr() == fz.clip_feat.data_ptr() + 100 * 512 * 2
    other = D.shard_features_16(fz, 0, 480, torch.bfloat16)  # another dtype is still a copy
    assert other.data_ptr() != fz.clip_feat.data_ptr() and other.dtype == torch.bfloat16


# ---- the stepped oracle is what it says it is -------------------------------------------------------------------------------
def test_stepped_oracle_is_self_consistent(oracle):
    """After one frame it is the fp32 oracle rounded to half; after two, a row hit twice is half(s2 * a + widen(h1) * b) in fp32
    with a = 1 / 2, b = 1 * a (clipfusion.py:716-720) and s2 the second frame's sample, a row hit once the rounded sample; every
    value is a half; the integer buffers are the fp32 oracle's."""
    w, h, dim = 64, 48, 64
    npy, npx = syn.feature_map_shape(w, h)
    grid = syn.make_grid((24, 20, 28))
    frames = syn.make_frames(77, 3, width=w, height=h, feat_dim=dim, npy=npy, npx=npx, depth_kind="B")[:2]
    args = lambda f: (f["depth"], f["rgb"], f["pose"], f["K"], f["feat"])
    new = lambda: oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, dim)
    only = [new(), new()]
    for v, f in zip(only, frames):
        v.integrate(*args(f))
    one = ref.stepped_oracle(oracle, grid, frames[:1], dim)
    assert torch.equal(one.clip_feat, only[0].clip_feat.half().float())
    two = ref.stepped_oracle(oracle, grid, frames, dim)
    both32 = new()
    for f in frames:
        both32.integrate(*args(f))
    for name in ("weight", "tsdf_weight", "tsdf", "rgb"):
        assert torch.equal(getattr(two, name), getattr(both32, name)), name
    assert torch.equal(two.clip_feat, two.clip_feat.half().float())
    w1, w2 = only[0].weight, only[1].weight
    twice, first, second = (w1 == 1) & (w2 == 1), (w1 == 1) & (w2 == 0), (w1 == 0) & (w2 == 1)
    assert int(twice.sum()) > 100 and int(first.sum()) > 100 and int(second.sum()) > 100
    a = torch.tensor(1.0) / torch.tensor(2.0)
    b = torch.tensor(1.0) * a
    want = (only[1].clip_feat[twice] * a + one.clip_feat[twice] * b).half().float()
    assert torch.equal(two.clip_feat[twice], want)
    assert torch.equal(two.clip_feat[first], one.clip_feat[first])
    assert torch.equal(two.clip_feat[second], only[1].clip_feat[second].half().float())
    # and it is NOT the fp32 result rounded once at the end (that is the bar of the order-free form, not of this one)
    assert not torch.equal(two.clip_feat[twice], both32.clip_feat[twice].half().float())


def test_edge_scene_taps_exactly_one_pixel(oracle):
    """The fp32 oracle on the rounding-edge scene: the 64 chosen voxels hold, after the one frame that hits, exactly the map
    pixel they project onto (the weights are {1, 0, 0, 0} with no rounding) -- so `expect32.half()` is `map.half()` at the tapped
    pixels, but for the negative zero (the blend adds +0 * 0) -- through a single frame and as frame 5 of 16."""
    for dim, n, hit in ((64, 1, 0), (512, 16, 5)):
        grid, frames, rows, expect32 = ref.edge_scene(dim, n, hit)
        vol = oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, dim)
        for f in frames:
            vol.integrate(f["depth"], f["rgb"], f["pose"], f["K"], f["feat"])
        assert int(vol.weight.max()) == 1 and bool((vol.weight[rows] == 1).all()) and len(rows) == 64
        got = vol.clip_feat[rows]
        assert torch.equal(got.view(torch.int32), expect32.view(torch.int32))
        fmap = frames[hit]["feat"][0]
        j = torch.arange(ref.EDGE_NP)
        jx, jy = torch.meshgrid(j, j, indexing="ij")
        tapped = fmap[:, jy.reshape(-1), jx.reshape(-1)].T
        neg_zero = (tapped == 0) & torch.signbit(tapped)
        same = ref.half_bits(expect32.half()) == ref.half_bits(tapped.half())
        assert bool((same | neg_zero).all()) and int(neg_zero.sum()) > 0 and bool((ref.half_bits(expect32.half())[neg_zero] == 0).all())
        # every edge value is among the expected halves, with the result the issue names for it
        hb = expect32.half()
        assert bool(torch.isinf(hb).any()) and bool((hb == -float("inf")).any())
        assert bool((hb == 65504.0).any()) and bool((hb == 1.0).any()) and bool((hb == 1.0 + 2.0 ** -9).any())
        sub = hb[(hb > 0) & (hb < 2.0 ** -14)]
        assert len(sub) > 0 and {float(v) for v in sub.unique()} == {float(torch.tensor(3e-6).half()), float(torch.tensor(6.1e-5).half())}
