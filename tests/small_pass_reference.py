"""NumPy statements of the five small device passes of csrc/saf_misc.hip, and the inputs their edge tests share.

The statements (label_argmax, scale, sample_vertices, backproject, clear_unwritten) say WHAT each pass computes, in the plainest
NumPy that says it; they share no code with oracle/saf_oracle.c.  tests/test_small_passes_host.py holds them against the CPU
oracle, tests/test_small_passes_gpu.py holds the HIP kernels against them.  Where a pass is one IEEE operation per value (scale)
or moves integers and bytes (argmax, clear, `valid`), the statement is exact and the comparison is bit for bit.  Where the kernel
chains fp32 operations (the trilinear blend, the back-projection) the statement works in float64 and returns, beside the value,
the magnitude the error bound is stated in:

    |got - want| <= 2^-20 * magnitude            (ERR_BOUND)

The blend has at most 11 fp32 roundings on the path of one term (two for the product of the three axis weights, one for the
multiplication by the value, up to eight additions), the back-projection at most 9; every rounding is at most 2^-24 of a partial
sum that the magnitude (the sum of the absolute terms) bounds, and 16 * 2^-24 = 2^-20 covers both.

Everything the kernel DECIDES with -- which corners lie in the volume, the nearest voxel, floor, the two axis weights -- is
computed here in float32, one rounded step at a time, as the kernel's comment fixes it (a float64 index would pick another
corner at a vertex that sits on a voxel boundary).
"""
import numpy as np

ERR_BOUND = 2.0 ** -20
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


# ------------------------------------------------------------------------------------------ the statements
def label_argmax(lab):
    """First index of the row maximum; -1 where the whole row is zero."""
    lab = np.asarray(lab).astype(np.int64)
    first_max = np.argmax(lab == lab.max(axis=1, keepdims=True), axis=1)
    return np.where((lab != 0).any(axis=1), first_max, -1).astype(np.int64)


def scale(feat, rgb, tsdf, weight, tsdf_weight, first, count, to_mean):
    """Sums -> means (x / w where w > 0, other rows left alone) or means -> sums (x * w, unconditionally) over voxels
    [first, first + count); `weight` scales features and rgb, `tsdf_weight` the tsdf.  Returns new (feat, rgb, tsdf)."""
    feat, rgb, tsdf = (np.array(a, dtype=np.float32, copy=True) for a in (feat, rgb, tsdf))
    rows = np.arange(first, first + count)
    w, wt = np.asarray(weight)[rows], np.asarray(tsdf_weight)[rows]
    with np.errstate(all="ignore"):
        if to_mean:
            a, b = rows[w > 0], rows[wt > 0]
            fw = np.asarray(weight)[a].astype(np.float32)
            feat[a] = feat[a] / fw[:, None]
            rgb[a] = rgb[a] / fw[:, None]
            tsdf[b] = tsdf[b] / np.asarray(tsdf_weight)[b].astype(np.float32)
        else:
            fw = w.astype(np.float32)
            feat[rows] = feat[rows] * fw[:, None]
            rgb[rows] = rgb[rows] * fw[:, None]
            tsdf[rows] = tsdf[rows] * wt.astype(np.float32)
    return feat, rgb, tsdf


def _wide(x):
    """A volume buffer as float64 (exact for fp32, bf16 and fp16; torch tensors because NumPy has no bf16)."""
    return x.double().numpy() if hasattr(x, "double") else np.asarray(x, dtype=np.float64)


def _axis(v, size):
    """The float32 steps of one axis: un-normalised index f, floor, the weights of corner floor and floor + 1."""
    f32 = np.float32
    v = np.asarray(v, dtype=f32)
    r = f32(1) / f32(size)
    g = (v + f32(0.5)) * r
    g = g * f32(2)
    g = g - f32(1)
    f = ((g + f32(1)) * f32(size) - f32(1)) / f32(2)
    fl = np.floor(f)
    w0 = (fl + f32(1)) - f
    w1 = f - fl
    assert f.dtype == f32 and w0.dtype == f32 and w1.dtype == f32
    return f, fl.astype(np.int64), w0, w1


def sample_vertices(feat, rgb, nvox, verts, obj_idx=None, seg_color=None):
    """3-D grid_sample(align_corners=False, zeros padding) of a [nx*ny*nz, .] volume at `verts` (voxel-index coordinates, in
    volume order x, y, z; the sampler's x runs along nz).  Returns a dict: feat / rgb (float64, rgb NOT yet clamped), feat_mag /
    rgb_mag (sum over the in-volume corners of |weight * value|), obj / seg (nearest, or None), and two masks per vertex:
    skipped (some corner lies outside the volume) and nearest_out (the nearest voxel does)."""
    nx, ny, nz = (int(n) for n in nvox)
    feat, rgb = _wide(feat), _wide(rgb)
    verts = np.asarray(verts, dtype=np.float32)
    ax = [_axis(verts[:, 2], nz), _axis(verts[:, 1], ny), _axis(verts[:, 0], nx)]  # sampler x, y, z
    size = (nz, ny, nx)
    nv = verts.shape[0]
    out = {"feat": np.zeros((nv, feat.shape[1])), "feat_mag": np.zeros((nv, feat.shape[1])), "rgb": np.zeros((nv, 3)),
           "rgb_mag": np.zeros((nv, 3)), "skipped": np.zeros(nv, dtype=bool)}
    for c in range(8):
        d = (c & 1, (c >> 1) & 1, c >> 2)
        idx = [ax[a][1] + d[a] for a in range(3)]
        inside = np.ones(nv, dtype=bool)
        for a in range(3):
            inside &= (idx[a] >= 0) & (idx[a] < size[a])
        out["skipped"] |= ~inside
        wgt = np.ones(nv)
        for a in range(3):
            wgt = wgt * (ax[a][3] if d[a] else ax[a][2]).astype(np.float64)
        row = (idx[2][inside] * ny + idx[1][inside]) * nz + idx[0][inside]
        for name, src in (("feat", feat), ("rgb", rgb)):
            term = wgt[inside, None] * src[row]
            out[name][inside] += term
            out[name + "_mag"][inside] += np.abs(term)
    near = [np.rint(ax[a][0]) for a in range(3)]  # float32, halves to even
    inside = np.ones(nv, dtype=bool)
    for a in range(3):
        inside &= (near[a] >= 0) & (near[a] < np.float32(size[a]))
    out["nearest_out"] = ~inside
    row = (near[2][inside].astype(np.int64) * ny + near[1][inside].astype(np.int64)) * nz + near[0][inside].astype(np.int64)
    out["obj"] = out["seg"] = None
    if obj_idx is not None:
        out["obj"] = np.zeros(nv, dtype=np.float32)
        out["obj"][inside] = np.asarray(obj_idx).reshape(-1)[row].astype(np.float32)
    if seg_color is not None:
        out["seg"] = np.zeros((nv, 3), dtype=np.float32)
        out["seg"][inside] = np.clip(np.asarray(seg_color, dtype=np.float32)[row], 0, 1)
    return out


def backproject(depth, pose, kinv, u_idx, v_idx, max_depth):
    """Lattice point o = j * nu + i is pixel (u_idx[i], v_idx[j]): xyz = R ((Kinv [u, v, 1]) d) + t in float64, the magnitude
    sum_j |R_ij| |d| sum_k |Kinv_jk p_k| + |t_i|, and valid = ~isnan(d) & (d > 0) & (d < max_depth) on the float32 depth."""
    depth = np.asarray(depth, dtype=np.float32)
    pose, kinv = np.asarray(pose, dtype=np.float64), np.asarray(kinv, dtype=np.float64)
    u = np.tile(np.asarray(u_idx, dtype=np.int64), len(v_idx))
    v = np.repeat(np.asarray(v_idx, dtype=np.int64), len(u_idx))
    d32 = depth[v, u]
    d = d32.astype(np.float64)
    p = np.stack([u, v, np.ones_like(u)], axis=1).astype(np.float64)  # [M, 3]
    rot, t = pose[:3, :3], pose[:3, 3]
    with np.errstate(all="ignore"):
        ray = p @ kinv.T
        xyz = (ray * d[:, None]) @ rot.T + t
        mag = ((np.abs(p)[:, None, :] * np.abs(kinv)[None]).sum(-1) * np.abs(d)[:, None]) @ np.abs(rot).T + np.abs(t)
        valid = ~np.isnan(d32) & (d32 > 0) & (d32 < np.float32(max_depth))
    return xyz, valid, mag


def clear_unwritten(feat_bytes, weight, first, n_rows):
    """Rows of [first, first + n_rows) whose weight is 0 become zero bytes; every other byte is kept."""
    out = np.array(feat_bytes, dtype=np.uint8, copy=True)
    rows = np.arange(first, first + n_rows)
    out[rows[np.asarray(weight)[rows] == 0]] = 0
    return out


# ------------------------------------------------------------------------------------------ shared inputs
GRID = (5, 7, 9)  # all three sides differ: a swap of two axes cannot hide
N_GRID = GRID[0] * GRID[1] * GRID[2]
ARGMAX_CLASSES = (1, 2, 63, 64, 65, 143, 200)


def argmax_planted(C):
    """(rows[int32, R x C], answer[R], names): the hand-made rows that fit into C classes, each with the index a
    reader can verify from the row's description (the statement is checked against these, too)."""
    rows, ans, names = [], [], []

    def add(name, row, a):
        rows.append(np.asarray(row, dtype=np.int64))
        ans.append(a)
        names.append(name)

    rng = np.random.default_rng(100 + C)
    bg = lambda: rng.integers(0, 10, C)  # a background of small counts
    add("all zero", np.zeros(C), -1)
    r = np.zeros(C); r[0] = 1; add("only class 0", r, 0)
    r = np.zeros(C); r[C - 1] = 1; add("only the last class", r, C - 1)
    r = -rng.integers(5, 1000, C); k = int(rng.integers(0, C)); r[k] = -2; add("all negative", r, k)
    r = np.full(C, I32_MIN); add("all INT32_MIN", r, 0)
    r = np.full(C, I32_MIN); r[C - 1] = I32_MIN + 1; add("INT32_MIN + 1 among INT32_MIN", r, C - 1)
    r = bg(); r[C // 2] = I32_MAX; add("INT32_MAX", r, C // 2)
    r = bg(); r[C - 1] = I32_MAX; r[0] = I32_MIN; add("INT32_MIN first, INT32_MAX last", r, C - 1)
    r = np.full(C, -7); r[C - 1] = -1; add("negative maximum in the last class", r, C - 1)
    if C >= 2:
        r = -rng.integers(1, 50, C); k = C // 3 + 1 if C > 2 else 1; r[k] = 0; r[C - 1] = 0
        add("zeros and negatives", r, k)
        r = np.full(C, I32_MIN); r[C - 1] = 0; r[C - 2] = -1; add("INT32_MIN, -1 and one zero", r, C - 1)
        r = np.full(C, -9); r[C - 2:] = -3; add("a negative maximum twice", r, C - 2)
        for c in sorted({0, C // 2 - 1 if C > 3 else 0, C - 2}):
            r = bg(); r[c] = r[c + 1] = 1000; add(f"tie at ({c}, {c + 1})", r, c)
        r = bg(); r[:] = 5; add("every class ties", r, 0)
    if C >= 65:
        r = bg(); r[63] = r[64] = 1000; add("tie at (63, 64)", r, 63)
        r = bg(); r[62] = r[63] = 1000; add("tie at (62, 63)", r, 62)
        for c in sorted({0, min(17, C - 65), C - 65}):
            r = bg(); r[c] = r[c + 64] = 1000; add(f"tie at ({c}, {c + 64})", r, c)
        r = bg(); r[C - 1] = r[C - 1 - 64] = I32_MAX; add("INT32_MAX tie 64 apart", r, C - 65)
    if C > 64 and C % 64:
        k = C - 1 - (C % 64) // 2  # inside the last, partial group of 64
        assert k >= (C // 64) * 64
        r = bg(); r[k] = 1000; add("maximum only in the last partial group", r, k)
        r = -rng.integers(5, 100, C); r[k] = -1; add("negative maximum only in the last partial group", r, k)
    if C > 128:
        r = bg(); r[3] = r[3 + 128] = 1000; add("tie at (3, 131)", r, 3)
    return np.stack(rows).astype(np.int32), np.asarray(ans, dtype=np.int64), names


def argmax_random(n_vox, C, seed):
    """Histogram-like rows: small counts (ties are the rule), a third of the rows empty, a tenth with negatives."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 4, (n_vox, C))
    kind = rng.integers(0, 10, n_vox)
    lab[kind < 3] = 0
    neg = kind == 9
    lab[neg] = -rng.integers(0, 4, (int(neg.sum()), C))
    return lab.astype(np.int32)


SCALE_WEIGHTS = np.array([0, 1, 2, 3, 7, 2 ** 24 + 1], dtype=np.int32)
SCALE_DIMS = (4, 6, 7, 512)


def scale_inputs(n, dim, seed):
    """A sum / mean volume of n voxels: finite nonzero data everywhere (also in rows of weight 0), the two weights drawn
    independently, NaN and inf planted in some rows whose weight is 0.  Rows 0, 1, n - 2 and n - 1 carry data and weight."""
    rng = np.random.default_rng(seed)
    feat = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
    feat[feat == 0] = 1.5
    rgb = rng.uniform(0.05, 1, (n, 3)).astype(np.float32)
    tsdf = rng.uniform(0.05, 1, n).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    weight = rng.choice(SCALE_WEIGHTS, n)
    tsdf_weight = rng.choice(SCALE_WEIGHTS, n)
    for k in (0, 1, n - 2, n - 1):
        weight[k], tsdf_weight[k] = 3, 7
    weight[n // 2], tsdf_weight[n // 2] = 7, 2  # (the one-voxel range)
    zero = np.nonzero(weight == 0)[0]
    feat[zero[0::3], 0] = np.nan
    feat[zero[1::3], dim - 1] = np.inf
    rgb[zero[1::3], 1] = -np.inf
    rgb[zero[0::3], 2] = np.nan
    zt = np.nonzero(tsdf_weight == 0)[0]
    tsdf[zt[0::3]] = np.nan
    tsdf[zt[1::3]] = np.inf
    return dict(feat=feat, rgb=rgb, tsdf=tsdf, weight=weight.astype(np.int32), tsdf_weight=tsdf_weight.astype(np.int32))


def scale_ranges(n):
    """(first, count): the whole volume, all but the two end voxels, one voxel, a range that ends at n."""
    return [(0, n), (1, n - 2), (n // 2, 1), (n - 9, 9)]


def same_bits(got, want):
    """float32 arrays equal bit for bit where neither is NaN, and NaN at the same places."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn]))


SAMPLE_DIMS = (3, 64, 70)  # below one wave, exactly one wave, a wave and a tail


def axis_values(n):
    return np.array([0, n - 1, 0.5, n - 1.5, 1, n - 2, -0.25, n - 0.75, -0.75, n - 0.25, 1.37, n - 1 - 1e-3, 1e-3], dtype=np.float32)


def sample_vertex_set(n_extra, seed=5):
    """(verts[float32, V x 3], n_planted): every combination of the per-axis edge coordinates, 500 random interior vertices,
    and n_extra more over the volume and a margin around it."""
    rng = np.random.default_rng(seed)
    ax = [axis_values(n) for n in GRID]
    planted = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)
    interior = rng.uniform(0, 1, (500, 3)) * (np.array(GRID) - 1)
    extra = rng.uniform(-1.0, 1.0, (n_extra, 3)) * (np.array(GRID) / 2 + 0.5) + (np.array(GRID) - 1) / 2
    return np.concatenate([planted, interior, extra]).astype(np.float32), len(planted)


def sample_volume(dim, seed=11):
    """float32 arrays of a GRID volume: features ~ 100 N(0, 1), rgb and seg_color in [-0.2, 1.2], obj_idx in [-50, 50]."""
    rng = np.random.default_rng(seed + dim)
    return dict(feat=(100 * rng.standard_normal((N_GRID, dim))).astype(np.float32),
                rgb=rng.uniform(-0.2, 1.2, (N_GRID, 3)).astype(np.float32),
                obj_idx=rng.integers(-50, 51, N_GRID).astype(np.int32),
                seg_color=rng.uniform(-0.2, 1.2, (N_GRID, 3)).astype(np.float32))


MAX_DEPTH = np.float32(3.7)
SPECIAL_DEPTHS = {"nan": np.float32(np.nan), "+0": np.float32(0.0), "-0": np.float32(-0.0), "-1": np.float32(-1.0),
                  "+inf": np.float32(np.inf), "max_depth": MAX_DEPTH, "below max_depth": np.nextafter(MAX_DEPTH, np.float32(0)),
                  "denormal": np.float32(1e-40)}
SPECIAL_VALID = {"nan": False, "+0": False, "-0": False, "-1": False, "+inf": False, "max_depth": False, "below max_depth": True,
                 "denormal": True}


def backproject_camera():
    """(pose[4,4], Kinv[3,3]) float32: a rotation about a skew axis, a translation, a K with different focal lengths."""
    a = np.array([0.3, -0.5, 0.8]); a /= np.linalg.norm(a)
    th = 0.9
    kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    rot = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    pose = np.eye(4); pose[:3, :3] = rot; pose[:3, 3] = (1.25, -0.75, 2.5)
    k = np.array([[8.1, 0.0, 4.3], [0.0, 7.9, 3.2], [0.0, 0.0, 1.0]])
    return pose.astype(np.float32), np.linalg.inv(k).astype(np.float32)


def backproject_cases():
    """[(name, depth[H,W] float32, u_idx, v_idx, {special name: lattice point})]."""
    rng = np.random.default_rng(21)
    small = rng.uniform(0.5, 5.0, (7, 9)).astype(np.float32)  # 9 wide, 7 high; some depths beyond max_depth
    where = {"nan": (0, 0), "+0": (1, 2), "-0": (6, 2), "-1": (3, 4), "+inf": (6, 8), "max_depth": (6, 5), "below max_depth": (0, 8),
             "denormal": (2, 8)}  # (v, u)
    for name, (v, u) in where.items():
        small[v, u] = SPECIAL_DEPTHS[name]
    big = rng.uniform(0.5, 5.0, (200, 300)).astype(np.float32)
    ub, vb = np.arange(2, 300, 7), np.arange(1, 200, 9)  # 43 x 23 = 989 points: three full blocks of 256 and a tail
    where_big = {name: (int(vb[3 + 2 * k]), int(ub[5 + 4 * k])) for k, name in enumerate(SPECIAL_DEPTHS)}
    where_big["nan"] = (int(vb[-1]), int(ub[-1]))  # the very last lattice point
    for name, (v, u) in where_big.items():
        big[v, u] = SPECIAL_DEPTHS[name]
    full = (np.arange(9), np.arange(7))
    cases = [("full grid", small, full[0], full[1]), ("one point", small, [4], [3]), ("repeated index", small, [2, 2, 5], [1, 6, 6]),
             ("last column", small, [8], full[1]), ("last row", small, full[0], [6]), ("last row and column", small, [0, 8, 8], [6, 0, 6]),
             ("300 x 200, 989 points", big, ub, vb)]
    out = []
    for name, depth, u, v in cases:
        u, v = np.asarray(u, dtype=np.int32), np.asarray(v, dtype=np.int32)
        w = where_big if depth is big else where
        hit = {}
        for s, (pv, pu) in w.items():
            js, is_ = np.nonzero(v == pv)[0], np.nonzero(u == pu)[0]
            if len(js) and len(is_):
                hit[s] = int(js[0]) * len(u) + int(is_[0])
        out.append((name, depth, u, v, hit))
    return out


CLEAR_SHAPES = [("f32", 3), ("f32", 4), ("f32", 8), ("f16", 5), ("bf16", 8), ("f16", 24), ("bf16", 36)]


def clear_inputs(n, row_bytes, seed):
    """(bytes[n, row_bytes] uint8, all nonzero; weight[n] int32): about half the rows unwritten, among them rows 0 and n - 1 and
    a run of 80 (a wave looks at 64 rows at a time: the run fills one ballot and parts of its neighbours)."""
    rng = np.random.default_rng(seed)
    data = (1 + (np.arange(n * row_bytes, dtype=np.int64) * 7 + 3) % 251).astype(np.uint8).reshape(n, row_bytes)
    weight = rng.integers(0, 2, n) * rng.integers(1, 5, n)
    run = min(100, max(0, n - 200))
    weight[run:run + 80] = 0
    weight[run + 80:run + 150] = 2  # and a run of written rows
    weight[0] = weight[n - 1] = 0
    weight[1] = 1
    weight[64:69] = (0, 0, 1, 0, 0)  # the range (65, 3): unwritten rows on both sides of it stay as they are
    return data, weight.astype(np.int32)


def clear_ranges(n):
    return [(0, n), (1, n - 2), (65, 3), (n // 3, 1)]
