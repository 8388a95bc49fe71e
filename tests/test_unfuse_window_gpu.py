"""GPU: fused frames taken out a window at a time (``deintegrate_features(..., windowed=True)``; include/saf.h:
saf_unfuse_frames_windowed -- the windowed path's classification and order-free row kernel of csrc/saf_window.hip run backwards).

What is promised bit for bit -- tsdf, tsdf_weight, weight, rgb, the label histograms and the two skip counters -- is compared with
a second module that removed the same frames through the per-frame pipeline (``windowed=False``); emptied voxels hold exact zero
rows either way.  The other feature rows are held to the bars of tests/deintegrate_reference.py against an oracle that never saw the
removed frames, and to a rounding-only bound of the same shape as its ``assert_rounding_only`` (``test_two_windows_...``).

64 x 48 frames from ``syn.make_frames``.  Each test prints its figures before it asserts; DESIGN 4.17 quotes them."""
import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd._lib import SafError

import deintegrate_reference as ref
from test_brick_form import _build, _frames, _fuse

pytestmark = pytest.mark.gpu

NVOX = (33, 30, 41)  # N = 40590: no multiple of the row kernel's 256-voxel piece; a lane's 4 voxels straddle the end
SEED = 9200          # (checked on the CPU: 4458 voxels emptied, 12404 keep two or more samples when 40 of the 60 frames leave)
BUFFERS = ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat")
EXACT = ("tsdf", "tsdf_weight", "weight", "rgb")  # (+ labels_one_hot): bit for bit the per-frame removal's
ROUNDINGS_WINDOWED = 16.0 * 2.0 ** -24

_cache = {}


def _grid(nvox=NVOX):
    return syn.make_grid(nvox, side=2.56 * nvox[0] / max(nvox))


def _module(grid, dim, seem, fdt=torch.float32, accum=_abi.SAF_RUNNING_MEAN):
    return _build(grid, dim, seem, accum, fdt, defer=False)


def _args(frames, seem):
    cat = lambda k: torch.cat([f[k] for f in frames]).cuda()
    labs = [f["labels"].float().cuda() for f in frames] if seem else None
    return (cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"), labs)


def _names(seem):
    return BUFFERS + (("labels_one_hot",) if seem else ())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _snapshot(fz, seem):
    return {name: getattr(fz, name).clone() for name in _names(seem)}


def _assert_same_bits(fz, snap, what, names=None):
    for name, t in snap.items():
        if names is None or name in names:
            assert torch.equal(_bits(getattr(fz, name)), _bits(t)), f"{name}: {what}"


def _take_out(fz, frames, seem, windowed, per_call=None, strict=False):
    per_call = per_call or len(frames)
    for s0 in range(0, len(frames), per_call):
        fz.deintegrate_features(*_args(frames[s0:s0 + per_call], seem), strict=strict, windowed=windowed)
    torch.cuda.synchronize()
    return fz


def _assert_against_oracle(fz, want, w, wt, k_w, k_t, seem, refilled=False):
    """The bars of tests/test_deintegrate_gpu.py, unchanged: index sets and histograms exact, tsdf / rgb within the CLOSE bar with
    the k w / (w - k) amplification, feature rows within 1e-4 of the row's largest magnitude."""
    assert torch.equal(fz.weight.cpu(), want.weight) and torch.equal(fz.tsdf_weight.cpu(), want.tsdf_weight), "index sets differ"
    if seem:
        assert torch.equal(fz.labels_one_hot.cpu(), want.labels_one_hot), "label histograms differ"
    return {"tsdf": ref.assert_value_bars(fz.tsdf.cpu().numpy(), want.tsdf.numpy(), wt, k_t, "tsdf", refilled),
            "rgb": ref.assert_value_bars(fz.rgb.cpu().numpy(), want.rgb.numpy(), w, k_w, "rgb", refilled),
            "clip_feat": ref.assert_feature_rows(fz.clip_feat.cpu().numpy(), want.clip_feat.numpy(), "clip_feat")}


def _scenario(oracle, key, nvox, dim, seem, kind, n_frames, out_idx, seed=SEED):
    """Frames, the oracle of all of them and of the ones that stay -- computed once, never modified."""
    if key not in _cache:
        grid = _grid(nvox)
        frames = _frames(seed, n_frames, dim, kind)
        out = set(out_idx)
        sc = {"grid": grid, "frames": frames, "removed": [frames[i] for i in sorted(out)],
              "all": ref.fuse_oracle(oracle, grid, frames, dim, seem),
              "kept": ref.fuse_oracle(oracle, grid, [f for i, f in enumerate(frames) if i not in out], dim, seem)}
        sc["w"], sc["wt"] = sc["all"].weight.numpy().astype(np.int64), sc["all"].tsdf_weight.numpy().astype(np.int64)
        sc["k_w"], sc["k_t"] = sc["w"] - sc["kept"].weight.numpy(), sc["wt"] - sc["kept"].tsdf_weight.numpy()
        sc["emptied"] = (sc["k_w"] > 0) & (sc["w"] == sc["k_w"])
        sc["two_left"] = (sc["k_w"] > 0) & (sc["w"] - sc["k_w"] >= 2)
        _cache[key] = sc
    return _cache[key]


def _main(oracle):
    return _scenario(oracle, "main", NVOX, 512, True, "B", 60, [i for i in range(60) if i % 3 != 0])


def _removed_windowed(sc, dim, seem):
    """Fuse the scenario's frames, take the removed ones out in ONE windowed call; the snapshot and the skip counters."""
    fz = _fuse(_module(sc["grid"], dim, seem), sc["frames"], seem)
    _take_out(fz, sc["removed"], seem, windowed=True)
    return fz


def _check_subset(sc, dim, seem, min_voxels):
    """Test 1's statement: bit for bit the per-frame removal where that is promised, the oracle's bars, exact zero rows."""
    n_empty, n_two = int(sc["emptied"].sum()), int(sc["two_left"].sum())
    print(f"{n_empty} voxels emptied, {n_two} keep two or more samples, largest weight {int(sc['w'].max())}")
    assert n_empty >= min_voxels and n_two >= min_voxels, "the test cannot pass on an empty intersection"
    fz = _removed_windowed(sc, dim, seem)
    twin = _take_out(_fuse(_module(sc["grid"], dim, seem), sc["frames"], seem), sc["removed"], seem, windowed=False)
    _assert_same_bits(fz, _snapshot(twin, seem), "differs from the per-frame removal's", EXACT + ("labels_one_hot",))
    used = _assert_against_oracle(fz, sc["kept"], sc["w"], sc["wt"], sc["k_w"], sc["k_t"], seem)
    twin_rows = ref.feature_row_error(twin.clip_feat.cpu().numpy(), sc["kept"].clip_feat.numpy())
    print(f"fraction of the bars used: {used}; the per-frame removal's feature rows: {twin_rows:.3g}")
    empty = torch.from_numpy(sc["emptied"])
    assert int(_bits(fz.clip_feat.cpu())[empty].abs().max()) == 0 and int(_bits(fz.rgb.cpu())[empty].abs().max()) == 0
    assert fz.stats()["deintegrate_skipped"] == {"valid": 0, "tsdf_valid": 0}
    # no counter of fusion moved: both modules fused alike, and neither removal touches stats[0..3], [5], [6] or [8..12]
    assert fz.stats() == twin.stats() and fz.stats()["frames"] == len(sc["frames"]) and fz.stats()["window_rows"] > 0
    return fz


# ---- 1. against the per-frame removal and the oracle ----------------------------------------------------------------------------
def test_forty_of_sixty_frames_leave_in_one_windowed_call(oracle):
    """Launches of 32 and 8 frames.  Measured: see DESIGN 4.17."""
    sc = _main(oracle)
    fz = _check_subset(sc, 512, True, 1000)
    _cache["main_bits"] = {name: t.cpu() for name, t in _snapshot(fz, True).items()}


# ---- 2. two windows, many hits per row -------------------------------------------------------------------------------------------
def _assert_rows_rounding_only(got, target, w, k, m_pre, m_samples, what):
    """``assert_rounding_only`` of tests/deintegrate_reference.py with the constant of the order-free op order:
    ``|got - target| <= 16 * 2^-24 * k * w / (w - k) * M`` per element, M over the row; exact zeros where ``w == k``."""
    got, target = np.asarray(got, dtype=np.float64), np.asarray(target, dtype=np.float64)
    w, k = np.asarray(w, dtype=np.float64), np.asarray(k, dtype=np.float64)
    big = np.maximum(np.asarray(m_pre, dtype=np.float64), np.asarray(m_samples, dtype=np.float64))
    left = w - k
    live = (left > 0) & (k > 0)
    bound = np.where(live, ROUNDINGS_WINDOWED * k * w / np.where(left > 0, left, 1.0), 0.0) * big
    err = np.abs(got - target)
    used = float((err[live] / np.maximum(bound[live], 1e-300)[:, None]).max(initial=0.0))
    print(f"{what}: largest error {float(err[live].max(initial=0.0)):.3g}, {used:.3g} of the rounding bound (c = 16), "
          f"largest k {int(k.max())}, largest w {int(w.max())}")
    assert not got[(left == 0) & (k > 0)].any(), f"{what}: an emptied row is not zero"
    assert used <= 1.0, f"{what}: {used:.3g} of the rounding bound"
    return used


def test_two_windows_of_a_camera_at_rest_round_only(oracle, monkeypatch):
    """150 frames, the camera at rest over frames 11 .. 111; frames 20 .. 119 leave in windows of 64 and 36 (SAF_WIN_FRAMES=64):
    rows with up to 92 hits in one removal.  From the device's own state before: tsdf and rgb under ``assert_rounding_only`` as it
    stands; feature rows under ``c * 2^-24 * k * w / (w - k) * M`` with c = 16 -- at most 12 k + 4 roundings per element: four
    chained FMAs per hit, the tap weights' scaling by 1 / w0, the oracle sample's own rounding, two roundings on the way out.
    Measured: see DESIGN 4.17."""
    monkeypatch.setenv("SAF_WIN_FRAMES", "64")
    dim, seem, grid = 256, False, _grid()
    frames = _frames(SEED + 2, 150, dim, "B", rest=(11, 112))
    removed = frames[20:120]
    rem = ref.removed_samples(oracle, grid, removed, dim, seem)
    fz = _fuse(_module(grid, dim, seem), frames, seem)
    pre = {name: t.cpu() for name, t in _snapshot(fz, seem).items()}
    target = ref.targets(type("Pre", (), pre), rem)
    _take_out(fz, removed, seem, windowed=True)
    w, wt = pre["weight"].numpy(), pre["tsdf_weight"].numpy()
    assert int(rem.k_w.max()) >= 80 and int((w - rem.k_w).min()) >= 0
    assert np.array_equal(fz.weight.cpu().numpy(), w - rem.k_w) and np.array_equal(fz.tsdf_weight.cpu().numpy(), wt - rem.k_t)
    untouched_w, untouched_t = torch.from_numpy(rem.k_w == 0), torch.from_numpy(rem.k_t == 0)
    for name, mask in (("tsdf", untouched_t), ("rgb", untouched_w), ("clip_feat", untouched_w)):
        assert torch.equal(_bits(getattr(fz, name).cpu())[mask], _bits(pre[name])[mask]), f"{name}: a voxel no removed frame hit was written"
    ref.assert_rounding_only(fz.tsdf.cpu().numpy(), target["tsdf"], wt, rem.k_t, pre["tsdf"].abs().numpy(), rem.m_tsdf, "tsdf")
    ref.assert_rounding_only(fz.rgb.cpu().numpy(), target["rgb"], w, rem.k_w, pre["rgb"].abs().numpy(), rem.m_rgb, "rgb")
    _assert_rows_rounding_only(fz.clip_feat.cpu().numpy(), target["clip_feat"], w, rem.k_w, pre["clip_feat"].abs().amax(dim=1).numpy(),
                               rem.m_feat, "clip_feat")
    assert fz.stats()["deintegrate_skipped"] == {"valid": 0, "tsdf_valid": 0}


# ---- 3. every width --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvox,dim,kind,n_frames,out_idx", [
    pytest.param((29, 33, 27), 768, "B", 20, [i for i in range(20) if i % 5 != 0], id="D768-16-of-20"),
    pytest.param((32, 16, 128), 1024, "A", 24, [i for i in range(24) if i % 7 not in (0, 3)], id="D1024-17-of-24-xcd-order"),
])
def test_the_other_widths(oracle, nvox, dim, kind, n_frames, out_idx):
    sc = _scenario(oracle, ("width", dim), nvox, dim, False, kind, n_frames, out_idx, seed=SEED + 3)
    assert len(sc["removed"]) >= 16
    _check_subset(sc, dim, False, 1)


# ---- 4. back to empty ------------------------------------------------------------------------------------------------------------
def test_every_frame_taken_out_again_leaves_a_fresh_volume(oracle):
    sc = _main(oracle)
    fz = _fuse(_module(sc["grid"], 512, True), sc["frames"], True)
    order = np.random.default_rng(5).permutation(60)
    _take_out(fz, [sc["frames"][i] for i in order], True, windowed=True, per_call=32)  # calls of 32 and 28
    _assert_same_bits(fz, _snapshot(_module(sc["grid"], 512, True), True), "differs from a freshly built module's")
    assert fz.stats()["deintegrate_skipped"] == {"valid": 0, "tsdf_valid": 0}


# ---- 5. the guard ----------------------------------------------------------------------------------------------------------------
def test_guard_the_same_frames_taken_out_twice(oracle):
    sc = _main(oracle)
    frames, seem = sc["frames"][:24], True
    twice = frames[:16]

    def run(windowed):
        fz = _fuse(_module(sc["grid"], 512, seem), frames, seem)
        _take_out(fz, twice, seem, windowed=windowed, strict=True)
        assert fz.stats()["deintegrate_skipped"] == {"valid": 0, "tsdf_valid": 0}
        if windowed:
            with pytest.raises(SafError, match="skipped"):  # (the removal has run when strict looks at the counters)
                _take_out(fz, twice, seem, windowed=True, strict=True)
        else:
            _take_out(fz, twice, seem, windowed=False)
        return fz

    a, b = run(True), run(False)
    sa, sb = a.stats()["deintegrate_skipped"], b.stats()["deintegrate_skipped"]
    print(f"skipped: windowed {sa}, per-frame {sb}")
    assert sa == sb and sa["valid"] > 0 and sa["tsdf_valid"] > 0
    _assert_same_bits(a, _snapshot(b, seem), "differs from the per-frame removal's", EXACT + ("labels_one_hot",))
    assert bool(torch.isfinite(a.clip_feat).all())
    assert int(_bits(a.clip_feat)[a.weight == 0].abs().max()) == 0, "a voxel of weight 0 holds a row that is not zero"
    assert int(a.weight.min()) >= 0 and int(a.tsdf_weight.min()) >= 0 and int(a.labels_one_hot.min()) >= 0


def test_guard_more_hits_in_one_window_than_the_voxel_holds():
    """k > w0 > 0: five frames of one pose and depth are fused, sixteen of that pose and depth are taken out in one window."""
    dim, seem, grid = 256, True, _grid()
    frames = _frames(SEED + 4, 16, dim, "B", rest=(0, 16))

    def run(windowed):
        fz = _fuse(_module(grid, dim, seem), frames[:5], seem)
        touched_w, touched_t = fz.weight.clone(), fz.tsdf_weight.clone()
        assert set(touched_w.unique().tolist()) == {0, 5} and set(touched_t.unique().tolist()) == {0, 5}
        _take_out(fz, frames, seem, windowed=windowed)
        return fz, int((touched_w == 5).sum()), int((touched_t == 5).sum())

    (a, n_w, n_t), (b, _, _) = run(True), run(False)
    assert n_w > 0 and n_t > 0
    assert int(a.weight.abs().max()) == 0 and int(a.tsdf_weight.abs().max()) == 0
    for name in ("clip_feat", "rgb", "tsdf", "labels_one_hot"):
        assert int(_bits(getattr(a, name)).abs().max()) == 0, f"{name} is not back in its constructed state"
    assert a.stats()["deintegrate_skipped"] == {"valid": 11 * n_w, "tsdf_valid": 11 * n_t} == b.stats()["deintegrate_skipped"]
    _assert_same_bits(a, _snapshot(b, seem), "differs from the per-frame removal's", EXACT + ("labels_one_hot", "clip_feat"))


# ---- 6. reproducible -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"SAF_WIN_OVERLAP": "0"}, {"SAF_WIN_XCD": "0"}], ids=["default", "one-stream", "linear-units"])
def test_the_windowed_removal_is_reproducible_bit_for_bit(oracle, monkeypatch, env):
    sc = _main(oracle)
    if "main_bits" not in _cache:
        _cache["main_bits"] = {name: t.cpu() for name, t in _snapshot(_removed_windowed(sc, 512, True), True).items()}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    again = _removed_windowed(sc, 512, True)
    for name, t in _cache["main_bits"].items():
        assert torch.equal(_bits(getattr(again, name).cpu()), _bits(t)), f"{name}: two runs differ"


# ---- 7. reintegrate --------------------------------------------------------------------------------------------------------------
def _perturbed(pose, rng):
    """A few centimetres and a few degrees off."""
    ang = np.deg2rad(rng.uniform(-3.0, 3.0, size=3))
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    rot = np.array([[cy * cz, -cy * sz, sy], [sx * sy * cz + cx * sz, -sx * sy * sz + cx * cz, -sx * cy],
                    [-cx * sy * cz + sx * sz, cx * sy * sz + sx * cz, cx * cy]])
    out = pose.clone()
    out[0, :3, :3] = torch.from_numpy(rot).float() @ pose[0, :3, :3]
    out[0, :3, 3] += torch.from_numpy(rng.uniform(-0.04, 0.04, size=3)).float()
    return out


def test_reintegrate_moves_thirty_two_frames_through_the_windowed_removal(oracle):
    sc = _main(oracle)
    grid, frames, dim, seem = sc["grid"], sc["frames"][:40], 512, True
    moved = [i for i in range(40) if i % 5 != 0]
    assert len(moved) == 32
    rng = np.random.default_rng(11)
    wrong = {i: _perturbed(frames[i]["pose"], rng) for i in moved}
    as_fused = [dict(f, pose=wrong[i]) if i in wrong else f for i, f in enumerate(frames)]
    fz = _fuse(_module(grid, dim, seem), as_fused, seem)
    depth, rgb, right, K, feat, labs = _args([frames[i] for i in moved], seem)
    old = torch.cat([wrong[i] for i in moved]).cuda()
    fz.reintegrate_features(depth, rgb, old, right, K, feat, labs, strict=True, windowed=True)
    torch.cuda.synchronize()
    want = ref.fuse_oracle(oracle, grid, frames, dim, seem)
    before = ref.fuse_oracle(oracle, grid, as_fused, dim, seem)
    without = ref.fuse_oracle(oracle, grid, [f for i, f in enumerate(frames) if i not in moved], dim, seem)
    w, wt = before.weight.numpy().astype(np.int64), before.tsdf_weight.numpy().astype(np.int64)
    used = _assert_against_oracle(fz, want, w, wt, w - without.weight.numpy(), wt - without.tsdf_weight.numpy(), seem, refilled=True)
    print(f"fraction of the bars used: {used}")
    assert fz.stats()["deintegrate_skipped"] == {"valid": 0, "tsdf_valid": 0}


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdt,accum", [pytest.param(torch.bfloat16, _abi.SAF_RUNNING_MEAN, id="bf16"),
                                       pytest.param(torch.float16, _abi.SAF_RUNNING_MEAN, id="fp16"),
                                       pytest.param(torch.float32, _abi.SAF_SUM, id="SAF_SUM")])
def test_16_bit_and_sum_volumes_are_refused_untouched(fdt, accum):
    dim, seem, grid = 512, True, _grid()
    frames = _frames(SEED, 16, dim, "B")
    fz = _fuse(_module(grid, dim, seem, fdt=fdt, accum=accum), frames[:7], seem)
    snap = {name: getattr(fz, name).clone() for name in _names(seem)}
    with pytest.raises(SafError):
        fz.deintegrate_features(*_args(frames, seem), windowed=True)
    with pytest.raises(SafError):
        fz.reintegrate_features(*_args(frames, seem)[:3], *_args(frames, seem)[2:], windowed=True)
    torch.cuda.synchronize()
    for name, t in snap.items():
        assert torch.equal(getattr(fz, name), t), f"{name} changed"


def test_a_width_without_a_backward_row_kernel():
    dim, seem, grid = 64, False, _grid()
    frames = _frames(SEED, 20, dim, "B")
    fz = _fuse(_module(grid, dim, seem), frames, seem)
    snap = _snapshot(fz, seem)
    with pytest.raises(SafError, match="saf_unfuse_path"):
        fz.deintegrate_features(*_args(frames[:16], seem), windowed=True)
    torch.cuda.synchronize()
    _assert_same_bits(fz, snap, "changed by a refused call")
    _take_out(fz, frames[:16], seem, windowed=None)  # the per-frame pipeline
    twin = _take_out(_fuse(_module(grid, dim, seem), frames, seem), frames[:16], seem, windowed=False)
    _assert_same_bits(fz, _snapshot(twin, seem), "windowed=None differs from windowed=False")
    assert int(fz.weight.max()) > 0
