"""NumPy restatement of the ray-cast contract (include/saf.h, saf_raycast), parameterised by dtype.

A helper, not a test file.  ``raycast(..., dtype=np.float32)`` follows the kernel operation for operation (every NumPy
ufunc call below is one IEEE operation of csrc/saf_raycast.hip, in its order); ``dtype=np.float64`` is the same chain in
double precision -- the reference the device is held to.  The inputs are the fp32 values the device sees (axis tables,
pose, K, step_vox, z_near, z_far as C floats) in both cases.

Also here: the scene and the views the ray-cast tests share, and the masks they compare on.
"""
import math

import numpy as np
import torch

from spatially_aware_ai_amd import synthetic as syn

MAX_SAMPLES = 65536


def _cell(g, n, T):
    i = np.clip(np.floor(g), 0, n - 2).astype(np.int64)  # (NaN never occurs for finite inputs)
    return i, g - i.astype(T)


def _lerp(a, b, f):
    d = b - a
    m = f * d
    return a + m


def _sample(tsdf, tw, nvox, gx, gy, gz, T):
    nx, ny, nz = nvox
    ix, fx = _cell(gx, nx, T)
    iy, fy = _cell(gy, ny, T)
    iz, fz = _cell(gz, nz, T)
    p00 = (ix * ny + iy) * nz + iz
    p01 = p00 + nz
    p10 = p00 + ny * nz
    p11 = p10 + nz
    c00 = _lerp(tsdf[p00], tsdf[p00 + 1], fz)
    c01 = _lerp(tsdf[p01], tsdf[p01 + 1], fz)
    c10 = _lerp(tsdf[p10], tsdf[p10 + 1], fz)
    c11 = _lerp(tsdf[p11], tsdf[p11 + 1], fz)
    c0 = _lerp(c00, c01, fy)
    c1 = _lerp(c10, c11, fy)
    f = _lerp(c0, c1, fx)
    obs = np.ones(gx.shape, dtype=bool)
    for p in (p00, p01, p10, p11):
        obs &= (tw[p] > 0) & (tw[p + 1] > 0)
    return f, obs


def _nearest(g, n):
    return np.clip(np.rint(g), 0, n - 1).astype(np.int64)  # rint: round half to even


def raycast(tsdf, tsdf_weight, axes, pose, K, height, width, step_vox=0.5, z_near=0.0, z_far=None, dtype=np.float64):
    """-> dict(depth [H,W] dtype, voxel [H,W] int64, hit [H,W] bool, k [H,W] int64 (crossing interval, -1 for a miss),
    step [H,W] dtype (the ray's sample step s))."""
    T = dtype
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    tsdf = f32(tsdf).astype(T)
    tw = np.asarray(tsdf_weight)
    ax = [f32(a) for a in axes]
    nvox = tuple(len(a) for a in ax)
    nx, ny, nz = nvox
    P = f32(pose).astype(T)
    Km = f32(K).astype(T)
    if z_far is None:
        z_far = grid_diagonal(float((ax[0][-1] - ax[0][0]) / (nx - 1)), nvox)
    step_vox, z_near, z_far = (T(np.float32(x)) for x in (step_vox, z_near, z_far))
    o3 = [T(a[0]) for a in ax]
    vs = (T(ax[0][-1]) - o3[0]) / T(nx - 1)
    v, u = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    u, v = u.reshape(-1).astype(T), v.reshape(-1).astype(T)
    dcx = (u - Km[0, 2]) / Km[0, 0]
    dcy = (v - Km[1, 2]) / Km[1, 1]
    d = [(P[a, 0] * dcx + P[a, 1] * dcy) + P[a, 2] for a in range(3)]
    og = [(P[a, 3] - o3[a]) / vs for a in range(3)]
    gd = [d[a] / vs for a in range(3)]
    npix = u.size
    tmin = np.full(npix, z_near, dtype=T)
    tmax = np.full(npix, z_far, dtype=T)
    ok = np.ones(npix, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            hi = T(nvox[a] - 1)
            nzero = gd[a] != 0
            t1 = (T(0) - og[a]) / gd[a]
            t2 = (hi - og[a]) / gd[a]
            tmin = np.where(nzero, np.maximum(tmin, np.minimum(t1, t2)), tmin)
            tmax = np.where(nzero, np.minimum(tmax, np.maximum(t1, t2)), tmax)
            ok &= nzero | ((og[a] >= 0) & (og[a] <= hi))
    ok &= tmin <= tmax
    if not (Km[0, 1] == 0 and Km[1, 0] == 0 and Km[2, 0] == 0 and Km[2, 1] == 0 and Km[2, 2] == 1):
        ok[:] = False
    dmax = np.maximum(np.maximum(np.abs(d[0]), np.abs(d[1])), np.abs(d[2]))
    s = (step_vox * vs) / dmax
    ok &= s > 0

    depth = np.zeros(npix, dtype=T)
    voxel = np.full(npix, -1, dtype=np.int64)
    hit_k = np.full(npix, -1, dtype=np.int64)
    live = np.nonzero(ok)[0]  # rays still marching
    prev_f = np.zeros(npix, dtype=T)
    prev_obs = np.zeros(npix, dtype=bool)
    for k in range(MAX_SAMPLES):
        if live.size == 0:
            break
        t = tmin[live] + T(k) * s[live]
        live = live[t <= tmax[live]]
        if live.size == 0:
            break
        t = tmin[live] + T(k) * s[live]
        f, obs = _sample(tsdf, tw, nvox, og[0] + t * gd[0][live], og[1] + t * gd[1][live], og[2] + t * gd[2][live], T)
        h = prev_obs[live] & obs & (prev_f[live] > 0) & (f <= 0)
        if h.any():
            r = live[h]
            t0 = tmin[r] + T(k - 1) * s[r]
            ts = t0 + s[r] * (prev_f[r] / (prev_f[r] - f[h]))
            vx = _nearest(og[0] + ts * gd[0][r], nx)
            vy = _nearest(og[1] + ts * gd[1][r], ny)
            vz = _nearest(og[2] + ts * gd[2][r], nz)
            depth[r] = ts
            voxel[r] = (vx * ny + vy) * nz + vz
            hit_k[r] = k - 1
        prev_f[live] = f
        prev_obs[live] = obs
        live = live[~h]
    shp = (height, width)
    return {"depth": depth.reshape(shp), "voxel": voxel.reshape(shp), "hit": (voxel >= 0).reshape(shp), "k": hit_k.reshape(shp),
            "step": s.reshape(shp)}


def grid_diagonal(voxel_size, nvox):
    """What ``render(z_far=None)`` uses: the length of the grid's diagonal."""
    return float(voxel_size) * math.sqrt(sum(float(n) ** 2 for n in nvox))


def fragile(r64, r32):
    """[H,W] bool: the float64 and float32 runs disagree on hit / miss, the crossing interval or the voxel."""
    return (r64["hit"] != r32["hit"]) | (r64["k"] != r32["k"]) | (r64["voxel"] != r32["voxel"])


def voxel_coords(voxel, nvox):
    nx, ny, nz = nvox
    return np.stack((voxel // (ny * nz), (voxel // nz) % ny, voxel % nz), axis=-1)


def point_in_grid(depth, axes, pose, K):
    """p(depth) in grid coordinates, in float64 from the fp32 inputs: [H,W,3]."""
    ax = [np.asarray(a, dtype=np.float32).astype(np.float64) for a in axes]
    P = np.asarray(pose, dtype=np.float32).astype(np.float64)
    Km = np.asarray(K, dtype=np.float32).astype(np.float64)
    h, w = depth.shape
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = np.stack(((u - Km[0, 2]) / Km[0, 0], (v - Km[1, 2]) / Km[1, 1], np.ones_like(u)), axis=-1)
    p = P[:3, 3] + np.asarray(depth, dtype=np.float64)[..., None] * (dc @ P[:3, :3].T)
    vs = (ax[0][-1] - ax[0][0]) / (len(ax[0]) - 1)
    return (p - np.array([a[0] for a in ax])) / vs


def constant_surface(surface, radius=2):
    """[H,W] bool: the analytic surface id is the same over the (2 radius + 1)^2 neighbourhood (no silhouette inside); the
    image border, whose neighbourhood is cut, is excluded."""
    s = np.asarray(surface)
    h, w = s.shape
    out = np.zeros((h, w), dtype=bool)
    core = np.ones((h - 2 * radius, w - 2 * radius), dtype=bool)
    c = s[radius:h - radius, radius:w - radius]
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            core &= s[radius + dy:h - radius + dy, radius + dx:w - radius + dx] == c
    out[radius:h - radius, radius:w - radius] = core
    return out


# ---- the scene and the views of tests/test_raycast_host.py and tests/test_raycast_gpu.py
NVOX, DIM, WH, N_FRAMES, SCAN_SEED = 64, 64, (160, 120), 60, 4242
TRUNC_VOX = 3.0


def scan():
    """60 look-at frames of the analytic scene (sphere r = 0.9 in a room of half-size 1.2; cameras at 2.5 m, outside the room)
    with the surface's class as label map and its class embedding (plus noise) as feature map."""
    w, h = WH
    return syn.SyntheticScan(SCAN_SEED, N_FRAMES, w, h, DIM)


def views():
    """Held-out cameras outside the room: [(name, pose [4,4] f32, K [3,3] f32)].  The camera of every view sits outside the
    room, so its rays cross the near wall from behind (a negative-to-positive crossing that must not be reported);
    'through_wall' looks square on through the middle of a wall with a long lens: every one of its rays crosses that wall's
    band from behind and then lands on the sphere -- there is no silhouette in the image, so the analytic depth bounds every
    pixel (at a silhouette the analytic depth jumps while the fused sphere is a fraction of a voxel fatter: the float64
    restatement itself reports 2 to 8 pixels per view nearer than their own analytic depth minus the truncation distance)."""
    w, h = WH
    out = []
    # One seed per view, so that a view can be replaced alone.  The seeds were chosen ON THE RESTATEMENT (float64 against
    # float32, and float64 against the analytic scene; tests/test_raycast_host.py re-checks all three conditions), never on the
    # device's output: (a) at most 1 % fragile pixels -- an un-rolled camera whose rays enter through a grid face puts every
    # other sample on a voxel plane, where floor() is a coin toss; (b) a 99th-percentile depth error inside the truncation
    # band -- the fused TSDF is projective, so along a ray that grazes a wall its zero set is off by (a fraction of a voxel) /
    # cos(incidence); (c) no hit in the two voxel planes that the grid keeps BEHIND the walls: seen from outside, the back edge
    # of a wall's band, which oblique frames carved to +1 and head-on frames left negative, is a front face of the fused field.
    for name, kind, kk, seed in (("look_at", "look_at", "centred", 22), ("rolled", "roll", "centred", 29),
                                 ("free_k", "roll", "free", 39), ("target", "target", "centred", 29)):
        gen = torch.Generator().manual_seed(seed)
        c = torch.randn(3, generator=gen, dtype=torch.float32)
        c = c / c.norm() * 2.5
        pose = syn.family_pose(gen, c, kind, target_radius=0.3)
        k = syn.intrinsics(w, h) if kk == "centred" else syn.family_intrinsics(gen, w, h)
        out.append((name, pose, k))
    k = syn.intrinsics(w, h)
    k[0, 0] = k[1, 1] = 2.0 * w  # half-angle to the image corner 17 degrees; the sphere subtends 22 from 2.4 m
    out.append(("through_wall", syn.look_at_pose(torch.tensor([2.4, 0.3, 0.2])), k))
    return out


def analytic(pose, k):
    """(depth [H,W] f32 numpy, surface [H,W] int64 numpy) of the analytic scene for a view; rays that leave the room backwards
    get depth 0."""
    w, h = WH
    depth, surface = syn._analytic_scene(pose, k, w, h)
    depth = torch.where(torch.isfinite(depth) & (depth > 0), depth, torch.zeros_like(depth))
    return depth.numpy(), surface.numpy()
