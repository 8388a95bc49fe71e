"""The NumPy float32 statement of saf_volume_resample (include/saf.h) that the tests of ``resample`` hold the device pass to.

A volume is a dict of arrays shaped by its grid, as in carry_reference.py, absorb_reference.py and coarsen_reference.py: ``tsdf`` f32,
``tsdf_weight``, ``weight`` i32 [nx,ny,nz], ``rgb`` f32 [nx,ny,nz,3], ``clip_feat`` [nx,ny,nz,D] and optionally ``labels_one_hot`` i32
[nx,ny,nz,C].  ``kind`` names the element type of ``clip_feat``: "f32", or "bf16" / "f16" (np.int16 bit patterns), widened and
narrowed by absorb_reference's helpers.  ``m12`` is the [3, 4] float32 matrix that takes a destination voxel's local index to a
continuous local index of the source box.  Every f32 operation of the device pass is one NumPy float32 operation here, in the same
order (corners in ascending k = 4 dx + 2 dy + dz), so every comparison against it is exact -- as long as no NaN is computed WITH.
``mean64`` is the float64 renormalised blend, ``matrix64`` the float64 mapping, and ``linear_bound`` the error bound of a linear
field, derived below from the statement's operation count."""
import numpy as np

from absorb_reference import narrow, widen

F32 = np.float32
U = 2.0 ** -24  # the unit roundoff of float32: one rounding errs by at most U times the result's magnitude


def matrix64(src_origin, src_vs, src_off, dst_origin, dst_vs, dst_off, transform=None):
    """The mapping in float64, evaluated at voxel centres as the statement says it: p(i) for the destination local indices 0, e_x,
    e_y, e_z, and from them the [3, 4] float64 matrix (p is affine in i)."""
    t = np.eye(4) if transform is None else np.asarray(transform, dtype=np.float64)
    inv = np.linalg.inv(t)

    def p(i):
        world_new = (np.asarray(i, np.float64) + np.asarray(dst_off, np.float64)) * float(dst_vs) + np.asarray(dst_origin, np.float64)
        world_old = inv[:3, :3] @ world_new + inv[:3, 3]
        return (world_old - np.asarray(src_origin, np.float64)) / float(src_vs) - np.asarray(src_off, np.float64)

    p0 = p((0, 0, 0))
    return np.stack([p((1, 0, 0)) - p0, p((0, 1, 0)) - p0, p((0, 0, 1)) - p0, p0], axis=1)


def footprint(m12, src_n, dst_n):
    """Per destination voxel (flattened, z fastest): ``any`` (the voxel has corners at all), and per corner k ``t`` [8, N] f32,
    ``inside`` [8, N] and the source flat index ``sv`` [8, N] (0 where the corner is not inside)."""
    m = np.asarray(m12, dtype=F32).reshape(3, 4)
    x, y, z = (g.reshape(-1) for g in np.meshgrid(*[np.arange(n, dtype=F32) for n in dst_n], indexing="ij"))
    lo, a0, a1 = [], [], []
    ok = np.ones(x.shape, dtype=bool)
    for a in range(3):
        p = (((m[a, 0] * x).astype(F32) + (m[a, 1] * y).astype(F32)).astype(F32) + (m[a, 2] * z).astype(F32)).astype(F32)
        p = (p + m[a, 3]).astype(F32)
        ok &= ~((p < F32(-1.0)) | (p >= F32(src_n[a])))  # compared in float, before any conversion
        fl = np.floor(p).astype(F32)
        f = (p - fl).astype(F32)
        lo.append(np.where(ok, fl, 0).astype(np.int64))
        a0.append((F32(1.0) - f).astype(F32))
        a1.append(f)
    t = np.zeros((8,) + x.shape, dtype=F32)
    inside = np.zeros((8,) + x.shape, dtype=bool)
    sv = np.zeros((8,) + x.shape, dtype=np.int64)
    for k in range(8):
        d = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        w = [a1[a] if d[a] else a0[a] for a in range(3)]
        t[k] = ((w[0] * w[1]).astype(F32) * w[2]).astype(F32)
        c = [lo[a] + d[a] for a in range(3)]
        inside[k] = ok & np.logical_and.reduce([(c[a] >= 0) & (c[a] < src_n[a]) for a in range(3)])
        sv[k] = np.where(inside[k], (c[0] * src_n[1] + c[1]) * src_n[2] + c[2], 0)
    return {"any": ok, "t": t, "inside": inside, "sv": sv}


def side(w, fp, min_cover):
    """One side of every destination voxel from the source's flat counts ``w``: ``on`` [8, N] (the contributing corners), K, S,
    ``seen`` (observed: K >= 1 and S >= min_cover), the stored count (the maximum, 0 where not observed) and ``best`` (the
    contributing corner with the largest t, the lowest k on a tie)."""
    on = fp["inside"] & (fp["t"] > 0) & (w[fp["sv"]] > 0)
    n = on.shape[1]
    s = np.zeros(n, dtype=F32)
    started = np.zeros(n, dtype=bool)
    wmax = np.zeros(n, dtype=np.int32)
    best, t_best = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=F32)
    for k in range(8):
        tk = fp["t"][k]
        s = np.where(on[k], np.where(started, (s + tk).astype(F32), tk), s)
        better = on[k] & (~started | (tk > t_best))
        best, t_best = np.where(better, k, best), np.where(better, tk, t_best)
        wmax = np.where(on[k], np.maximum(wmax, w[fp["sv"][k]]), wmax)
        started |= on[k]
    count = on.sum(0)
    seen = (count >= 1) & (s >= F32(min_cover))
    return {"on": on, "K": count, "S": s, "seen": seen, "count": np.where(seen, wmax, 0).astype(np.int32), "best": best}


def blend(x, fp, sd):
    """The K >= 2 case on the source's flat values ``x`` [Ns, C] (float32): r = 1 / S, c_k = t_k * r, acc = x_1 * c_1, acc = acc +
    x_k * c_k.  Where K < 2 the result means nothing."""
    n = sd["on"].shape[1]
    with np.errstate(all="ignore"):
        r = (F32(1.0) / np.where(sd["K"] >= 2, sd["S"], F32(1.0))).astype(F32)
        acc = np.zeros((n, x.shape[1]), dtype=F32)
        started = np.zeros(n, dtype=bool)
        for k in range(8):
            on = sd["on"][k]
            if not on.any():
                continue
            ck = (fp["t"][k] * r).astype(F32)
            p = (np.where(on[:, None], x[fp["sv"][k]], F32(0)).astype(F32) * ck[:, None]).astype(F32)
            new = np.where(started[:, None], (acc + p).astype(F32), p)
            acc = np.where(on[:, None], new, acc)
            started |= on
    return acc


def only_corner(raw, fp, sd):
    """The K == 1 case (and the label row of any observed voxel): the bytes of the heaviest contributing corner of ``raw`` [Ns, C]."""
    return raw[np.take_along_axis(fp["sv"], sd["best"][None, :], axis=0)[0]]


def mean64(x, fp, sd):
    """The float64 blend over the contributing corners, renormalised: sum t_k x_k / sum t_k with the statement's f32 t_k widened;
    NaN where no corner contributes."""
    num = np.zeros((sd["on"].shape[1], x.shape[1]), dtype=np.float64)
    den = np.zeros(sd["on"].shape[1], dtype=np.float64)
    for k in range(8):
        on = sd["on"][k]
        tk = np.where(on, fp["t"][k].astype(np.float64), 0.0)
        num += np.where(on[:, None], x[fp["sv"][k]].astype(np.float64), 0.0) * tk[:, None]
        den += tk
    with np.errstate(all="ignore"):
        return num / den[:, None]


def resample(src, dst_n, m12, min_cover=0.5, kind="f32", dst=None):
    """The destination volume and (rows blended, rows copied, tsdf voxels blended, tsdf voxels copied).  ``dst``: what the
    destination held before -- its feature and label rows stay where the feature side is not observed (default: zeros); the small
    fields are written everywhere.  No value of a corner that does not contribute is used."""
    src_n = src["weight"].shape
    dst_n = tuple(int(v) for v in dst_n)
    fp = footprint(m12, src_n, dst_n)
    flat = lambda a: a.reshape((-1,) + a.shape[3:])
    sf, st = side(flat(src["weight"]), fp, min_cover), side(flat(src["tsdf_weight"]), fp, min_cover)
    sel = lambda sd, one, many, none: np.where((sd["seen"] & (sd["K"] == 1))[:, None], one,
                                               np.where((sd["seen"] & (sd["K"] >= 2))[:, None], many, none))
    grid = lambda a: a.reshape(dst_n + a.shape[1:])
    out = {"weight": grid(sf["count"]), "tsdf_weight": grid(st["count"])}
    # ---- the TSDF side
    t = flat(src["tsdf"])[:, None]
    out["tsdf"] = grid(sel(st, only_corner(t, fp, st), blend(t, fp, st), F32(0))[:, 0].astype(F32))
    # ---- the feature side
    c = flat(src["rgb"])
    out["rgb"] = grid(sel(sf, only_corner(c, fp, sf), blend(c, fp, sf), F32(0)).astype(F32))
    rows = flat(src["clip_feat"])
    keep = np.zeros((fp["any"].size, rows.shape[1]), dtype=rows.dtype) if dst is None else flat(dst["clip_feat"])
    out["clip_feat"] = grid(sel(sf, only_corner(rows, fp, sf), narrow(blend(widen(rows, kind), fp, sf), kind), keep).astype(rows.dtype))
    if "labels_one_hot" in src:
        lab = flat(src["labels_one_hot"])
        keep = np.zeros((fp["any"].size, lab.shape[1]), dtype=np.int32) if dst is None else flat(dst["labels_one_hot"])
        out["labels_one_hot"] = grid(np.where(sf["seen"][:, None], only_corner(lab, fp, sf), keep).astype(np.int32))
    blended = lambda sd: int((sd["seen"] & (sd["K"] >= 2)).sum())
    copied = lambda sd: int((sd["seen"] & (sd["K"] == 1)).sum())
    return out, (blended(sf), copied(sf), blended(st), copied(st))


def voxel_mix(src, dst_n, m12, min_cover=0.5):
    """What a case exercises.  Per side ("weight", "tsdf_weight"): the destination voxels [N] that are ``blended`` (observed,
    K >= 2), ``copied`` (observed, K == 1) and ``gated`` (not observed although K >= 1), as masks; ``outside``: the voxels with no
    corner at all; ``all_inside``: those whose eight corners all lie inside the source box; and ``either``: per kind, the number
    of voxels that are of that kind on at least one side."""
    fp = footprint(m12, src["weight"].shape, dst_n)
    out = {"outside": int((~fp["any"]).sum()), "all_inside": fp["inside"].all(0), "voxels": int(fp["any"].size)}
    for name in ("weight", "tsdf_weight"):
        sd = side(src[name].reshape(-1), fp, min_cover)
        out[name] = {"blended": sd["seen"] & (sd["K"] >= 2), "copied": sd["seen"] & (sd["K"] == 1), "gated": ~sd["seen"] & (sd["K"] >= 1),
                     "seen": sd["seen"], "K": sd["K"]}
    out["either"] = {kind: int((out["weight"][kind] | out["tsdf_weight"][kind]).sum()) for kind in ("blended", "copied", "gated")}
    return out


def linear_bound(m12, dst_n, grad_index, x_max):
    """The bound [N] on |blend - field at the destination centre| for a source whose values are an affine field rounded to
    float32, at destination voxels all of whose eight corners are observed (so every p_a >= 0 and f_a = p_a - floor(p_a) is exact).
    ``grad_index``: the field's gradient per SOURCE voxel index, [C, 3]; ``x_max``: the largest magnitude of the source's values,
    [C].  Computed from the inputs alone, with u = 2^-24:

      * the position.  The device works at p^ = p + dp: an entry of m12 is the float64 entry rounded once (u), a product
        m_ak * (float)x is rounded (u), and each of the three sums is rounded on a partial sum of magnitude at most
        P_a = |m_a0| x + |m_a1| y + |m_a2| z + |m_a3| (u each): |dp_a| <= 5 u P_a, 6 u P_a with the second-order terms.  Exact
        trilinear weights at p^ reproduce a linear field at p^, so this costs sum_a |grad_a| 6 u P_a.
      * the weights.  1.0f - f is one rounding (u), t_k = (a_x a_y) a_z two more on top of its three factors: t^_k = t_k (1 + e),
        |e| <= 5 u.  S adds up to eight of them (7 roundings on partial sums <= 1, and sum t^ = 1 + 5 u), r = 1 / S and
        c_k = t_k r are one rounding each: c_k = t_k (1 + e_k) with |e_k| <= 5 u + 5 u + 7 u + 2 u = 19 u.
      * the blend.  A product x_k c_k is one rounding, the 7 sums one each on partial sums of at most sum |c_k x_k|: 8 u;
        the source value itself is the field rounded once: u.
      In all (19 + 8 + 1) u sum |c_k x_k|, 29 u with the second-order terms, and sum |c_k x_k| <= max |x| (1 + 19 u)."""
    m = np.abs(np.asarray(m12, dtype=np.float64).reshape(3, 4))
    x, y, z = (g.reshape(-1) for g in np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dst_n], indexing="ij"))
    p_mag = np.stack([m[a, 0] * x + m[a, 1] * y + m[a, 2] * z + m[a, 3] for a in range(3)], axis=1)  # [N, 3]
    g = np.abs(np.asarray(grad_index, dtype=np.float64))  # [C, 3]
    return 6 * U * (p_mag @ g.T) + 29 * U * np.asarray(x_max, dtype=np.float64)[None, :]
