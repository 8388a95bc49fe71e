"""The yardsticks of the de-integration tests (``deintegrate`` / ``reintegrate``, include/saf.h: saf_unfuse_frames), on the CPU.

A fused volume keeps per voxel a running mean ``m`` of ``w`` samples.  Taking ``k`` of them (sum ``S``) out again leaves, in exact
arithmetic, ``(w m - S) / (w - k)`` -- ``float64_target``.  Two statements are checked against it:

* against an oracle that never saw the removed frames (``assert_value_bars``): the project's CLOSE bar, 1e-4 relative + 1e-6
  absolute, with the absolute part carrying the derived amplification -- an error ``d`` in a mean of ``w`` samples becomes
  ``d w / (w - k)`` after ``k`` removals, and each removal adds one rounding of the same size: ``1e-6 k w / (w - k)``.  A voxel no
  removed frame hit (``k = 0``) holds what forward fusion left there -- the rounding-only test asserts that it is bit for bit the
  state before -- and keeps the plain CLOSE bar the forward tests hold it to (read literally the formula leaves it no absolute part;
  measured, the subset test's inputs pass that reading too: no such element is over 1e-4 |want|); a voxel that lost every
  sample (``w = k``) must hold exact zeros.  Feature rows: largest error over the row's largest magnitude <= 1e-4, the measure and
  bar of tests/test_sums_form.py.
* a rounding-only statement from the device's own state before the removal (``assert_rounding_only``):
  ``|got - target| <= 15 * 2^-24 * k * w / (w - k) * M`` with ``M`` the largest magnitude among the state before and the removed
  samples (over the row for a feature row): about 5 roundings per removal (reciprocal, b, two products, the difference), each
  scaled by at most (w + 1) / (w - 1) <= 3.

The removed frames' per-voxel samples come from fusing each frame ALONE into an empty ``OracleVolume``: where its count is 1 the
stored value is the sample (s * 1 + 0 * 0).
"""
from dataclasses import dataclass

import numpy as np
import torch

RTOL, ATOL, FEAT_REL = 1e-4, 1e-6, 1e-4
ROUNDINGS = 15.0 * 2.0 ** -24


def float64_target(w, m, s_sum, k):
    """``(w m - S) / (w - k)`` in float64; exactly 0 where ``w == k``.  ``w``, ``k`` [N]; ``m``, ``s_sum`` [N] or [N, C]."""
    w, k = np.asarray(w, dtype=np.float64), np.asarray(k, dtype=np.float64)
    m, s_sum = np.asarray(m, dtype=np.float64), np.asarray(s_sum, dtype=np.float64)
    if m.ndim == 2:
        w, k = w[:, None], k[:, None]
    left = w - k
    return np.where(left > 0, (w * m - s_sum) / np.where(left > 0, left, 1.0), 0.0)


def amplification(w, k, refilled=False):
    """``k w / (w - k)`` where samples are left and some were removed, 1 where none was removed, 0 where none is left --
    ``refilled`` (reintegrate: frames were fused again afterwards): 1 there too, an emptied voxel restarts from exact zeros."""
    w, k = np.asarray(w, dtype=np.float64), np.asarray(k, dtype=np.float64)
    left = w - k
    return np.where(left > 0, np.where(k > 0, k * w / np.where(left > 0, left, 1.0), 1.0), 1.0 if refilled else 0.0)


def value_errors(got, want, w, k, refilled=False):
    """Per element: |got - want| and what the bar allows (0 where the voxel is empty again: exact zeros)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    amp = amplification(w, k, refilled)
    if got.ndim == 2:
        amp = amp[:, None]
    allowed = np.where(amp > 0, RTOL * np.abs(want) + ATOL * amp, 0.0)
    return np.abs(got - want), allowed


def assert_value_bars(got, want, w, k, what, refilled=False):
    """tsdf / rgb of test 2.  Returns the largest error as a fraction of what the bar allows (for the record)."""
    err, allowed = value_errors(got, want, w, k, refilled)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), f"{what}: non-finite values"
    used = float((err / np.maximum(allowed, 1e-300))[allowed > 0].max(initial=0.0))
    print(f"{what}: largest error {float(err.max(initial=0.0)):.3g}, {used:.3g} of the bar")
    bad = err > allowed
    assert not bad.any(), f"{what}: {int(bad.sum())} elements over the bar, worst {float(err[bad].max()):.3g} (allowed {float(allowed[bad].min()):.3g})"
    return used


def feature_row_error(got, want):
    """Largest error of a row over the row's largest magnitude (tests/test_sums_form.py), worst row."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.maximum(np.abs(want).max(axis=-1, keepdims=True), 1e-30)
    return float((np.abs(got - want) / scale).max(initial=0.0))


def assert_feature_rows(got, want, what):
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all(), f"{what}: non-finite values"
    worst = feature_row_error(got, want)
    print(f"{what}: largest row error {worst:.3g} of the row's largest magnitude")
    assert worst <= FEAT_REL, f"{what}: error {worst:.3g} of the row's largest magnitude (allowed {FEAT_REL})"
    return worst


@dataclass
class Removed:
    """What a set of frames put into each voxel: how many of them hit it, the float64 sums and largest magnitudes of their samples."""
    k_w: np.ndarray       # [N] frames that hit the voxel on the weight side (valid)
    k_t: np.ndarray       # [N] ... on the tsdf_weight side (tsdf-valid)
    s_tsdf: np.ndarray    # [N]
    s_rgb: np.ndarray     # [N, 3]
    s_feat: np.ndarray    # [N, D]
    m_tsdf: np.ndarray    # [N] largest |sample|
    m_rgb: np.ndarray     # [N, 3]
    m_feat: np.ndarray    # [N] largest |sample| over the row and the frames
    labels: np.ndarray    # [N, n_classes] votes, or None


def frames_alone(oracle, grid, frames, dim, seem):
    """Fuse each frame ALONE into an empty ``OracleVolume`` and yield ``(frame, volume, hit_w, hit_t)``: where the volume's
    count is 1 (``hit_w`` on the weight side, ``hit_t`` on the tsdf_weight side) its stored values are the frame's samples
    (s * 1 + 0 * 0).  The loop ``removed_samples`` and tests/feature_family_reference.py share."""
    for f in frames:
        one = oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, dim, 143 if seem else 0)
        one.integrate(f["depth"], f["rgb"], f["pose"], f["K"], f["feat"], [f["labels"].float()] if seem else None, rgb_bilinear=seem)
        hit_w, hit_t = one.weight.numpy() == 1, one.tsdf_weight.numpy() == 1
        assert int(one.weight.max()) <= 1 and int(one.tsdf_weight.max()) <= 1
        yield f, one, hit_w, hit_t


def removed_samples(oracle, grid, frames, dim, seem):
    """Fuse each frame alone into an empty ``OracleVolume``; where its count is 1 the stored values are the frame's samples."""
    n = int(np.prod([int(v) for v in grid.nvox]))
    r = Removed(np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n), np.zeros((n, 3)), np.zeros((n, dim)), np.zeros(n),
                np.zeros((n, 3)), np.zeros(n), np.zeros((n, 143), np.int64) if seem else None)
    for _, one, hit_w, hit_t in frames_alone(oracle, grid, frames, dim, seem):
        r.k_w += hit_w
        r.k_t += hit_t
        r.s_tsdf += one.tsdf.numpy().astype(np.float64)  # (zero where the frame did not hit)
        r.m_tsdf = np.maximum(r.m_tsdf, np.abs(one.tsdf.numpy()))
        r.s_rgb += one.rgb.numpy().astype(np.float64)
        r.m_rgb = np.maximum(r.m_rgb, np.abs(one.rgb.numpy()))
        rows = np.flatnonzero(hit_w)
        feat = one.clip_feat.numpy()[rows].astype(np.float64)
        r.s_feat[rows] += feat
        r.m_feat[rows] = np.maximum(r.m_feat[rows], np.abs(feat).max(axis=1))
        if seem:
            r.labels += one.labels_one_hot.numpy()
    return r


def targets(pre, rem):
    """float64 targets of tsdf, rgb and the feature rows from a state ``pre`` (anything with the volume's buffer names, device
    tensors or an ``OracleVolume``) and what the removed frames put in."""
    g = lambda name: getattr(pre, name).detach().cpu().numpy()
    return {
        "tsdf": float64_target(g("tsdf_weight"), g("tsdf"), rem.s_tsdf, rem.k_t),
        "rgb": float64_target(g("weight"), g("rgb"), rem.s_rgb, rem.k_w),
        "clip_feat": float64_target(g("weight"), g("clip_feat"), rem.s_feat, rem.k_w),
    }


def assert_rounding_only(got, target, w, k, m_pre, m_samples, what):
    """``|got - target| <= 15 * 2^-24 * k * w / (w - k) * M``; exact zeros where ``w == k``; untouched (bit for bit the state before,
    which the caller checks) where ``k == 0``.  Returns the largest error as a fraction of the bound."""
    got, target = np.asarray(got, dtype=np.float64), np.asarray(target, dtype=np.float64)
    w, k = np.asarray(w, dtype=np.float64), np.asarray(k, dtype=np.float64)
    big = np.maximum(np.asarray(m_pre, dtype=np.float64), np.asarray(m_samples, dtype=np.float64))
    left = w - k
    amp = np.where((left > 0) & (k > 0), ROUNDINGS * k * w / np.where(left > 0, left, 1.0), 0.0)
    bound = (amp[:, None] if big.ndim == 2 else amp) * big
    if got.ndim == 2 and bound.ndim == 1:
        bound = bound[:, None]
    err = np.abs(got - target)
    touched = np.broadcast_to((k > 0)[:, None] if got.ndim == 2 else (k > 0), got.shape)
    used = float((err / np.maximum(bound, 1e-300))[touched & (bound > 0)].max(initial=0.0))
    print(f"{what}: largest error {float(err[touched].max(initial=0.0)):.3g}, {used:.3g} of the rounding bound")
    bad = touched & (err > bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements over the rounding bound, worst {float((err / np.maximum(bound, 1e-300))[bad].max()):.3g} of it"
    return used


def fuse_oracle(oracle, grid, frames, dim, seem, poses=None):
    vol = oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, dim, 143 if seem else 0)
    cat = lambda key: torch.cat([f[key] for f in frames])
    vol.integrate(cat("depth"), cat("rgb"), cat("pose") if poses is None else poses, cat("K"), cat("feat"),
                  [f["labels"].float() for f in frames] if seem else None, rgb_bilinear=seem)
    return vol
