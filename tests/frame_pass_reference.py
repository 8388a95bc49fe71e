"""Plain statements of the frame-side passes: the 7 x 7 depthwise convolution (csrc/saf_dwconv.hip), the tile front-end and the
staging copy (csrc/saf_misc.hip) and the packed merge (csrc/saf_merge.hip).  tests/test_frame_passes_host.py holds them against
the library on the CPU; the four GPU files hold the HIP kernels against them.

Where a kernel chains fp32 operations the statement works in float64 and returns, beside the value, the magnitudes the error
bound is stated in; the bounds are derived from the kernels' operation counts, never from their output:

  dwconv, fp32    |got - exact| <= 50 * 2^-24 * S,  S = |b| + sum |x * w| over the taps inside the image.  The kernel does 49 fmaf
                  into an fp32 accumulator that starts at the bias: an output passes through at most 49 roundings, each at most
                  2^-24 of a partial sum that S bounds.
  tiles           |got - want| <= 2^-21 * (p * R + 2 * M) per pixel; R = max - min and M = the largest magnitude of the pixel's
                  four normalised taps.  A source coordinate is below p and carries at most two fp32 roundings on either side
                  (the compiler may fuse the multiply and the subtraction), so a weight differs by at most 2^-22 * p per axis, and
                  the blend is continuous across a change of i0; the normalisation and the blend add a few roundings of M.  A
                  wrong tap costs about R times a weight.

Everything the tile kernel DECIDES with -- the source coordinate, i0, i1 and the two weights -- is computed here in float32, one
rounded step at a time.  The staging and merge statements move bytes or add in rank order: they are exact.
"""
import numpy as np
import torch

DWCONV_BOUND = 50.0 * 2.0 ** -24
TILE_BOUND = 2.0 ** -21
GUARD = 64  # guard elements before and after a guarded destination

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


# ------------------------------------------------------------------------------------------ depthwise convolution
def dwconv7x7_f64(x, w, b=None):
    """x [N, C, H, W], w [C, 1, 7, 7], b [C] or None (any float dtype, any device) -> (exact, S) as float64 CPU tensors
    [N, C, H, W]: the zero-padded 7 x 7 depthwise convolution and the per-element sum of its absolute terms."""
    x, w = x.detach().cpu().double(), w.detach().cpu().double()
    n, c, h, wd = x.shape
    xp = torch.zeros((n, c, h + 6, wd + 6), dtype=torch.float64)
    xp[:, :, 3:3 + h, 3:3 + wd] = x
    b = torch.zeros(c, dtype=torch.float64) if b is None else b.detach().cpu().double()
    exact = b.view(1, c, 1, 1).expand(n, c, h, wd).clone()
    mag = exact.abs()
    for ky in range(7):
        for kx in range(7):
            term = xp[:, :, ky:ky + h, kx:kx + wd] * w[:, 0, ky, kx].view(1, c, 1, 1)  # (a tap outside the image: 0 in both)
            exact += term
            mag += term.abs()
    return exact, mag


def ulp16_fraction(y32, dtype):
    """Where each fp32 value lies between its two 16-bit neighbours, in units of the 16-bit ulp: 0 = representable, 0.5 = a tie
    (values in the normal range of `dtype`; 0 for zeros)."""
    drop = 16 if dtype == torch.bfloat16 else 13
    bits = y32.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & ((1 << drop) - 1)
    return bits.double() / float(1 << drop)


# ------------------------------------------------------------------------------------------ tiles
def _axis_f32(p, out):
    """ATen's align_corners=False source index for one axis, in float32 and unfused: (i0, i1, l0, l1)."""
    f32 = np.float32
    scale = f32(p) / f32(out)
    o = np.arange(out, dtype=np.float32)
    t = o + f32(0.5)
    t = (scale * t).astype(np.float32)
    f = (t - f32(0.5)).astype(np.float32)
    f = np.where(f < 0, f32(0), f).astype(np.float32)
    i0 = f.astype(np.int64)
    i1 = np.minimum(i0 + 1, p - 1)
    l1 = (f - i0.astype(np.float32)).astype(np.float32)
    l0 = (f32(1) - l1).astype(np.float32)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def tiles_f64(rgb, patch, stride, out, mean=CLIP_MEAN, std=CLIP_STD):
    """rgb [B, 3, H, W] in 0..1 -> (tiles, R, M), float64 arrays [B * npy * npx, 3, out, out]: normalise, unfold into patch x patch
    tiles at `stride`, resize every tile bilinearly to out x out (align_corners=False).  mean / std are taken as the float32
    values the kernel receives."""
    x = np.asarray(rgb, dtype=np.float32).astype(np.float64)
    bsz, _, h, w = x.shape
    assert patch <= h and patch <= w and (h - patch) % stride == 0 and (w - patch) % stride == 0
    m = np.asarray(mean, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    s = np.asarray(std, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    x = (x - m) / s
    npy, npx = 1 + (h - patch) // stride, 1 + (w - patch) // stride
    i0, i1, l0, l1 = _axis_f32(patch, out)
    y0, y1, x0, x1 = i0[:, None], i1[:, None], i0[None, :], i1[None, :]
    h0, h1, w0, w1 = l0[:, None], l1[:, None], l0[None, :], l1[None, :]
    shape = (bsz * npy * npx, 3, out, out)
    tiles, rng, mag = (np.empty(shape, dtype=np.float64) for _ in range(3))
    t = 0
    for b in range(bsz):
        for py in range(npy):
            for px in range(npx):
                pt = x[b, :, py * stride:py * stride + patch, px * stride:px * stride + patch]
                v00, v01, v10, v11 = pt[:, y0, x0], pt[:, y0, x1], pt[:, y1, x0], pt[:, y1, x1]
                tiles[t] = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11)
                taps = np.stack([v00, v01, v10, v11])
                rng[t] = taps.max(axis=0) - taps.min(axis=0)
                mag[t] = np.abs(taps).max(axis=0)
                t += 1
    return tiles, rng, mag


def tile_error_ratio(got, want, rng, mag, patch):
    """Largest |got - want| / E over all pixels, E = 2^-21 * (p * R + 2 * M)."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float((err / (TILE_BOUND * (patch * rng + 2.0 * mag))).max())


# ------------------------------------------------------------------------------------------ staging
def guarded(shape, fill, device, count=1):
    """`count` destinations of `shape` in ONE flat float buffer, GUARD elements before, between and after them, everything
    `fill`: (buffer, [views]).  A view starts GUARD + i * (numel + GUARD) elements in: off a 16-byte boundary for odd sizes and
    odd i, as the slots of a batch are."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + count * (n + GUARD),), float(fill), dtype=torch.float32, device=device)
    views = [buf[GUARD + i * (n + GUARD):GUARD + i * (n + GUARD) + n].view(shape) for i in range(count)]
    return buf, views


def stage_expected(buf, views, sources, fill):
    """What a guarded buffer holds after staging: sources[i] (None: nothing is copied) as a contiguous copy in slot i, `fill`
    everywhere else.  Exact."""
    want = torch.full_like(buf, float(fill))
    n = views[0].numel()
    for i, s in enumerate(sources):
        if s is not None:
            o = GUARD + i * (n + GUARD)
            want[o:o + n] = s.contiguous().reshape(-1)
    return want


# ------------------------------------------------------------------------------------------ packed merge
def merge_positions(w):
    """pos[i] = touched rows (weight > 0) among [0, i), i = 0 .. n: int32 [n + 1]."""
    return torch.cat([torch.zeros(1, dtype=torch.int64, device=w.device), torch.cumsum(w > 0, 0)]).int()


def merge_expected(t, w, first, n_rows, recv=None, world=0):
    """Without `recv`: the packed send buffer, the touched rows of t[first : first + n_rows] in order.  With recv [world * mine
    rows]: t after the add -- every touched row of the range replaced by its `world` contributions added left to right."""
    idx = torch.nonzero(w > 0).squeeze(1)
    sel = idx[(idx >= first) & (idx < first + n_rows)]
    if recv is None:
        return t[sel]
    ref = t.clone()
    mine = len(sel)
    if mine:
        parts = recv.view((world, mine) + tuple(t.shape[1:]))
        acc = parts[0].clone()
        for k in range(1, world):
            acc = acc + parts[k]
        ref[sel] = acc
    return ref
