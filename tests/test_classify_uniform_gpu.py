"""GPU: the window classification's frame loop at the small shapes where a wave-uniform loop can go wrong (csrc/saf_window.hip,
`classify_bricks_kernel` / `classify_voxels`): the loop runs on the wave's mask of live frames held in a scalar register, and a
frame's depth pointer and camera come by scalar loads.  So: bricks that are whole padding (no live frame at all), bricks cut at
each upper face, launches of 16 / 17 / 32 / 1 frames, live masks with holes, with a single bit and with only the top bit, frames
that every brick culls, non-finite depth, and the camera families -- on every route the kernel is launched from.

Against the CPU oracle: weight, tsdf_weight and the valid / tsdf-valid counters exactly; tsdf and rgb at the tolerance of
tests/test_gpu_parity.py, feature rows at that of tests/test_sums_form.py (1e-4 of the row's largest magnitude); the cull
counters must show that each reason fired and that every (brick, frame) pair was tested once."""
import pytest
import torch

from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd import synthetic as syn

from test_brick_form import EXACT, _build, _feat_close, _fuse
from test_gpu_parity import _close

pytestmark = pytest.mark.gpu

W, H, DIM = 64, 48, 256  # the smallest image the suite's windowed cases use, the row kernel's smallest width
# neither grid is a multiple of the 4 x 4 x 16 brick on any axis: 6 x 4 (x 3) brick columns leave 40 of an 8 x 8 tile's 64 as
# padding; the second has nz % 4 != 0 (a lane's four voxels cut by the upper z face: the scalar TSDF loads and stores)
GRID_A, GRID_B = (22, 14, 40), (21, 13, 38)
REASONS = ("behind", "far", "frustum", "occluded")


def _bricks(nvox):
    return -(-nvox[0] // 4) * -(-nvox[1] // 4) * -(-nvox[2] // 16)


def _away(frame):
    """The frame's camera at 2.5 m from the grid with its back to it: every brick is behind it."""
    c = frame["pose"][0, :3, 3]
    pose = syn.look_at_pose(c / c.norm() * 2.5)
    pose[:3, 0] = -pose[:3, 0]  # half a turn about the camera's down axis (a rotation still)
    pose[:3, 2] = -pose[:3, 2]
    return dict(frame, pose=pose[None])


def _outside(frame):
    """A look-at camera 2.5 m away, so that a depth image of zeros puts every brick beyond its largest depth."""
    c = frame["pose"][0, :3, 3]
    return dict(frame, pose=syn.look_at_pose(c / c.norm() * 2.5)[None], K=syn.intrinsics(W, H)[None], depth=torch.zeros(1, H, W))


def _scan(n, cameras):
    """`n` frames; every 16 of them hold one camera that looks away, one image of zeros, one with +inf and NaN pixels and one
    long lens, so that the live masks have holes.  65 frames: the second launch keeps its LAST frame only (bit 31 alone), the third is one frame."""
    npy, npx = syn.feature_map_shape(W, H)
    if cameras == "look_at":
        frames = syn.make_frames(5100 + n, n, width=W, height=H, feat_dim=DIM, npy=npy, npx=npx, depth_kind="B", missing_depth_frac=0.05)
    else:
        frames = syn.make_family_frames(5200 + n, n, W, H, DIM, npy, npx)
    for i in range(n):
        if i % 16 == 1 or (n == 65 and 32 <= i < 63 and i % 2 == 0):
            frames[i] = _away(frames[i])
        elif i % 16 == 2 or (n == 65 and 32 <= i < 63):
            frames[i] = _outside(frames[i])
        elif i % 16 == 3:
            d = frames[i]["depth"].clone()
            d[:, ::5, ::3] = float("inf")
            d[:, 1::7, ::4] = float("nan")
            frames[i] = dict(frames[i], depth=d)
        elif i % 16 == 4:  # a long lens: the grid's outer bricks lie outside the frustum, whatever the camera family
            k = frames[i]["K"].clone()
            k[0, 0, 0], k[0, 1, 1] = 4.0 * W, 4.0 * W
            frames[i] = dict(frames[i], K=k)
        elif cameras == "skew" and i % 16 == 5:  # skew and a scaled rotation: no cull applies, the pixel boundaries move
            pose, k = frames[i]["pose"].clone(), frames[i]["K"].clone()
            pose[0, :3, :3] *= 1.05
            k[0, 0, 1] = 3.0
            frames[i] = dict(frames[i], pose=pose, K=k)
    return frames


_REF = {}


def _reference(oracle, nvox, n, cameras, accum=_abi.SAF_RUNNING_MEAN):
    """(grid, frames, the oracle's volume), computed once and shared."""
    key = (nvox, n, cameras, accum)
    if key not in _REF:
        grid = syn.make_grid(nvox, side=2.56 * nvox[0] / max(nvox))
        frames = _scan(n, cameras)
        vol = oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, DIM, 0, accum)
        cat = lambda k: torch.cat([f[k] for f in frames])
        vol.integrate(cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"))
        _REF[key] = (grid, frames, vol)
    return _REF[key]


def _check(fz, vol, nvox, n, reasons=REASONS, tsdf=True):
    st = fz.stats()
    c = st["cull"]
    print(f"{nvox} x {n} frames: valid {st['valid']} tsdf_valid {st['tsdf_valid']} cull {c}")
    assert st["window_rows"] > 0, "the windowed path did not run"
    assert torch.equal(fz.weight.cpu(), vol.weight), "valid voxel sets differ from the oracle's"
    assert torch.equal(fz.tsdf_weight.cpu(), vol.tsdf_weight), "tsdf-valid voxel sets differ from the oracle's"
    assert st["valid"] == int(vol.stats[0]) > 0 and st["tsdf_valid"] == int(vol.stats[1]) > 0
    assert st["frames"] == n
    assert c["pairs"] == _bricks(nvox) * n, "every (brick, frame) pair is tested once; a brick in the padding tests none"
    for r in reasons:
        assert c[r] > 0, f"no (brick, frame) pair was dropped as '{r}' ({c})"
    assert sum(c[r] for r in REASONS) < c["pairs"]
    if tsdf:
        _close(fz.tsdf, vol.tsdf, "tsdf")
    _close(fz.rgb, vol.rgb, "rgb")
    _feat_close(fz.clip_feat, vol.clip_feat, 1e-4, "clip_feat vs the oracle")
    return st


@pytest.mark.parametrize("nvox,n", [(GRID_A, 16), (GRID_A, 17), (GRID_A, 32), (GRID_A, 33), (GRID_A, 65), (GRID_B, 33)])
def test_frames_per_launch_and_partial_bricks(oracle, nvox, n):
    """Calls of 16, 17, 32, 33 and 65 frames: launches of 16, 17, 32, 32 + 1 and 32 + 32 + 1 frames."""
    grid, frames, vol = _reference(oracle, nvox, n, "look_at")
    fz = _fuse(_build(grid, DIM, False, _abi.SAF_RUNNING_MEAN, torch.float32), frames, False)
    _check(fz, vol, nvox, n)


@pytest.mark.parametrize("cameras", ["family", "skew"])
def test_camera_families(oracle, monkeypatch, cameras):
    """Rolled / off-centre cameras (every cull active), and among them cameras with skew and a scaled rotation (no cull)."""
    monkeypatch.setenv("SAF_CLS_VERIFY", "1")
    grid, frames, vol = _reference(oracle, GRID_A, 33, cameras)
    fz = _fuse(_build(grid, DIM, False, _abi.SAF_RUNNING_MEAN, torch.float32), frames, False)
    _check(fz, vol, GRID_A, 33)
    assert int(fz.fuse_stats[7]) == 0, "the guarded pixel path disagrees with the reference's chain"


ROUTES = {
    "sum": (_abi.SAF_SUM, {}),
    "tiled": (_abi.SAF_RUNNING_MEAN, {"SAF_TILED_MIN_VOXELS": "0", "SAF_CLS_TILED": "2"}),  # ... forced for the first unit too
    "untiled": (_abi.SAF_RUNNING_MEAN, {"SAF_CLS_TILED": "0"}),
    "verify": (_abi.SAF_RUNNING_MEAN, {"SAF_CLS_VERIFY": "1"}),
    "verify_tiled": (_abi.SAF_SUM, {"SAF_CLS_VERIFY": "1", "SAF_TILED_MIN_VOXELS": "0", "SAF_CLS_TILED": "2"}),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_routes(oracle, monkeypatch, route):
    """The kernel's instantiations: running mean and SAF_SUM, tiled depth copies on and off, the self-checking form."""
    accum, env = ROUTES[route]
    grid, frames, vol = _reference(oracle, GRID_A, 33, "family", accum)
    # SAF_SUM: the TSDF is compared bit for bit with the per-frame pipeline below
    one = _fuse(_build(grid, DIM, False, accum, torch.float32, defer=False), frames, False, per_call=7)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fz = _fuse(_build(grid, DIM, False, accum, torch.float32), frames, False)
    _check(fz, vol, GRID_A, 33, tsdf=accum == _abi.SAF_RUNNING_MEAN)
    for name in EXACT:
        assert torch.equal(getattr(fz, name), getattr(one, name)), f"{name} differs from the per-frame pipeline"
    if "SAF_CLS_VERIFY" in env:
        assert int(fz.fuse_stats[7]) == 0, "the guarded pixel path disagrees with the reference's chain"


def test_two_frames_in_flight_update_the_tsdf_in_frame_order(oracle):
    """The loop projects and gathers two frames before it updates the TSDF with either.  Six consecutive frames from ONE camera,
    their depth images a fifth of the truncation band apart: every voxel near the surface is updated by both frames of a pair
    with different values, so the running mean depends on the order -- bit for bit the per-frame pipeline's, frame after frame."""
    grid = syn.make_grid(GRID_A, side=2.56 * GRID_A[0] / max(GRID_A))
    frames = _scan(33, "look_at")
    for i in range(7, 13):
        frames[i] = dict(frames[i], pose=frames[6]["pose"], K=frames[6]["K"], depth=frames[6]["depth"] + (i - 6) * 0.2 * grid.trunc)
    vol = oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, DIM, 0, _abi.SAF_RUNNING_MEAN)
    cat = lambda k: torch.cat([f[k] for f in frames])
    vol.integrate(cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"))
    one = _fuse(_build(grid, DIM, False, _abi.SAF_RUNNING_MEAN, torch.float32, defer=False), frames, False, per_call=7)
    fz = _fuse(_build(grid, DIM, False, _abi.SAF_RUNNING_MEAN, torch.float32), frames, False)
    _check(fz, vol, GRID_A, 33)
    both = (vol.tsdf_weight >= 6).sum()
    assert int(both) > 500, "too few voxels are updated by all the frames of the camera at rest"
    for name in EXACT:
        assert torch.equal(getattr(fz, name), getattr(one, name)), f"{name} differs from the per-frame pipeline"


def test_session_pushes_of_32_equal_one_call(oracle):
    """One frame per call: the queue pushes the frames into a streaming session 32 at a time, each push one classification launch
    through the same launcher as a call's.  Bit for bit the one call of 65 frames, and the oracle's sets."""
    grid, frames, vol = _reference(oracle, GRID_A, 65, "look_at")
    bulk = _fuse(_build(grid, DIM, False, _abi.SAF_RUNNING_MEAN, torch.float32), frames, False)
    fed = _fuse(_build(grid, DIM, False, _abi.SAF_RUNNING_MEAN, torch.float32), frames, False, per_call=1)
    _check(fed, vol, GRID_A, 65)
    for name in EXACT + ("clip_feat",):
        assert torch.equal(getattr(fed, name), getattr(bulk, name)), f"{name}: pushes of 32 differ from one call"
    sf, sb = fed.stats(), bulk.stats()
    assert sf["cull"] == sb["cull"] and all(sf[k] == sb[k] for k in ("valid", "tsdf_valid", "frames"))
