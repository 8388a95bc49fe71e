"""GPU: a second fused volume of the same lattice absorbed (``absorb``; include/saf.h: saf_volume_absorb, csrc/saf_absorb.hip).

(a), (b): the device pass against its NumPy restatement (tests/absorb_reference.py) on random buffers, byte for byte.
(c): a volume that holds ONE frame, absorbed, is that frame fused -- equal as values; the TSDF within the project's 1e-4, because
the forward sweep divides with the hardware reciprocal and the pass by IEEE division.
(d): two scans fused separately and joined against one module that fused all the frames: counts exact, running means within the
bar the project uses wherever the order of summation changes (1e-4 of the row's largest magnitude; two partial means combined
round differently from one running mean -- 0.67 n 2^-24 at n <= 40 in NumPy); what only one of the two touched is that one's, bit
for bit.  (e): 16-bit modules against the restatement applied to their own buffers, bit for bit.  (f), (g): stale rows, queues."""
import ctypes as C

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd._lib import check, lib

import absorb_reference as ref
from test_brick_form import _feat_close
from test_carry_gpu import BOX_A, BOX_B, H, NAMES, TORCH_DT, W, _bits, _descriptor, _fuse, _module, _names, _one_by_one, _scan, \
    _to_device

pytestmark = pytest.mark.gpu

KIND = {_abi.SAF_F32: "f32", _abi.SAF_BF16: "bf16", _abi.SAF_F16: "f16"}
KIND_OF = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
BIG = (1 << 24) + 1  # a count that (float) rounds: to even, 2^24
LABEL_POISON, LABEL_SENTINEL = -(1 << 30), -9
FORCED = ((2, 7), (3, 0), (0, 5), (0, 0))  # (ws, wd) of an overlap's first voxels: blend, copy, nothing written (twice)


# ---- (a) the pass on random buffers -------------------------------------------------------------------------------------------
def _overlap_voxels(ov, k):
    """The first ``k`` voxels of the flattened overlap as flat indices into (the destination, the source)."""
    d, s = ov
    ext = tuple(sl.stop - sl.start for sl in d)
    k = min(k, int(np.prod(ext)))
    ijk = np.stack(np.unravel_index(np.arange(k), ext), axis=1)
    return ijk + np.array([sl.start for sl in d]), ijk + np.array([sl.start for sl in s])


def _random_pair(s_n, d_n, off, dim, dt, classes, rng):
    """CPU tensors of a source and a destination.  The four weight arrays are drawn independently from {0, 1 .. 300}, about half
    zeros; an overlap's first voxels are forced through the states (both sides, the TSDF side in reverse order), and the fifth has
    a destination count of 2^24 + 1.  Then the poison: whatever belongs to a voxel whose count is 0 -- the row, rgb, tsdf -- is NaN
    (labels: a poison value in the source, a sentinel in the destination)."""
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    vols = []
    for nvox in (s_n, d_n):
        n = int(np.prod(nvox))
        draw = lambda: torch.from_numpy((rng.integers(0, 2, n) * rng.integers(1, 301, n)).astype(np.int32))
        v = {"tsdf": torch.randn(n, generator=g), "tsdf_weight": draw(), "weight": draw(), "rgb": torch.rand(n, 3, generator=g),
             "clip_feat": torch.randn(n, dim, generator=g).to(TORCH_DT[dt])}
        if classes:
            v["labels_one_hot"] = torch.from_numpy(rng.integers(0, 50, (n, classes)).astype(np.int32))
        vols.append(v)
    src, dst = vols
    ov = ref.overlap(s_n, d_n, off)
    if ov is not None:
        dv, sv = _overlap_voxels(ov, 5)
        for j, (d_ijk, s_ijk) in enumerate(zip(dv, sv)):
            di, si = np.ravel_multi_index(tuple(d_ijk), d_n), np.ravel_multi_index(tuple(s_ijk), s_n)
            if j < 4:
                src["weight"][si], dst["weight"][di] = FORCED[j]
                src["tsdf_weight"][si], dst["tsdf_weight"][di] = FORCED[3 - j] if len(dv) >= 4 else FORCED[j]
            else:
                src["weight"][si], dst["weight"][di] = 1, BIG
                src["tsdf_weight"][si], dst["tsdf_weight"][di] = 3, BIG
    for v, lab in ((src, LABEL_POISON), (dst, LABEL_SENTINEL)):
        v["clip_feat"][v["weight"] == 0] = float("nan")
        v["rgb"][v["weight"] == 0] = float("nan")
        v["tsdf"][v["tsdf_weight"] == 0] = float("nan")
        if classes:
            v["labels_one_hot"][v["weight"] == 0] = lab
    return src, dst


def _grids(v, nvox, kind):
    """NumPy copies shaped by the grid, as absorb_reference takes them: f32 as values, 16-bit rows as bit patterns."""
    out = {}
    for k, t in v.items():
        t = t.detach().cpu()
        if k == "clip_feat" and kind != "f32":
            t = t.view(torch.int16)
        out[k] = t.numpy().reshape(tuple(nvox) + tuple(t.shape[1:])).copy()
    return out


def _np_bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


S, D_ = (9, 7, 13), (12, 5, 20)
PASS_CASES = [
    # src, dst, off, D, dtype, classes, misaligned (0 no, 1 destination, 2 source) -- the shapes of test_carry_gpu.py's PASS_CASES
    pytest.param(S, D_, (-2, 1, -5), 512, _abi.SAF_F32, 143, 0, id="D512-f32-labels"),
    pytest.param(S, D_, (3, -1, 4), 8, _abi.SAF_F32, 0, 0, id="D8-f32"),
    pytest.param(S, D_, (0, 0, 0), 6, _abi.SAF_F32, 143, 0, id="D6-f32-24-byte-rows-labels"),
    pytest.param(S, D_, (8, 6, 12), 512, _abi.SAF_BF16, 143, 0, id="one-voxel-bf16"),
    pytest.param(S, D_, (2, 4, 10), 512, _abi.SAF_F16, 0, 0, id="63-voxels-fp16"),
    pytest.param(S, D_, (5, 3, 9), 512, _abi.SAF_F32, 143, 0, id="64-voxels"),
    pytest.param(S, D_, (4, 6, 0), 12, _abi.SAF_F16, 143, 0, id="65-voxels-D12-fp16-24-byte-rows"),
    pytest.param(S, D_, (20, 0, 0), 8, _abi.SAF_F32, 143, 0, id="disjoint"),
    pytest.param(S, D_, (-2, 1, -5), 512, _abi.SAF_BF16, 0, 0, id="D512-bf16"),
    pytest.param(S, D_, (3, -1, 4), 512, _abi.SAF_F16, 143, 0, id="D512-fp16-labels"),
    pytest.param(S, (5, 3, 6), (2, 2, 3), 512, _abi.SAF_BF16, 0, 0, id="crop-bf16"),
    pytest.param((5, 3, 6), S, (-2, -2, -3), 8, _abi.SAF_F32, 143, 0, id="grow"),
    pytest.param(S, D_, (-2, 1, -5), 512, _abi.SAF_F32, 0, 1, id="D512-f32-destination-off-16-bytes"),
    pytest.param(S, D_, (3, -1, 4), 512, _abi.SAF_F16, 143, 2, id="D512-fp16-source-off-16-bytes"),
    pytest.param(S, D_, (3, -1, 4), 512, _abi.SAF_BF16, 0, 1, id="D512-bf16-destination-off-16-bytes"),
]
N_OVERLAP = {"one-voxel-bf16": 1, "63-voxels-fp16": 63, "64-voxels": 64, "65-voxels-D12-fp16-24-byte-rows": 65, "disjoint": 0}


@pytest.mark.parametrize("s_n,d_n,off,dim,dt,classes,misaligned", PASS_CASES)
def test_pass_equals_its_restatement_and_touches_nothing_else(request, s_n, d_n, off, dim, dt, classes, misaligned):
    kind = KIND[dt]
    rng = np.random.default_rng(abs(hash((s_n, d_n, off, dim, dt))) % (1 << 32))
    src, dst = _random_pair(s_n, d_n, off, dim, dt, classes, rng)
    before_s, before_d = _grids(src, s_n, kind), _grids(dst, d_n, kind)
    m = ref.written_masks(before_s, before_d, off)
    case = request.node.callspec.id
    if case in N_OVERLAP:
        assert int(m["inside"].sum()) == N_OVERLAP[case]
    if m["inside"].sum() >= 8:  # a condition of the test: all four (ws, wd) states, on both sides, and the rounding count
        ov = ref.overlap(s_n, d_n, off)
        for side in ("weight", "tsdf_weight"):
            ws, wd = before_s[side][ov[1]], before_d[side][ov[0]]
            for a in (False, True):
                for b in (False, True):
                    assert (((ws > 0) == a) & ((wd > 0) == b)).any(), (side, a, b)
            assert (wd == BIG).any() and ((wd == BIG) & (ws > 0)).any()
    elif m["inside"].sum() >= 1:
        assert m["blend"].any() and m["t_blend"].any(), "a tiny overlap's first voxel is blended"
    want, inc = ref.absorb(_grids(src, s_n, kind), _grids(dst, d_n, kind), off, kind)
    s_dev, d_dev = _to_device(src, misaligned == 2), _to_device(dst, misaligned == 1)
    counts = torch.tensor([5, 7, 11, 13], dtype=torch.int64, device="cuda")
    vs, vd = _descriptor(s_dev, s_n, dim, dt), _descriptor(d_dev, d_n, dim, dt)
    check(lib().saf_volume_absorb(C.byref(vs), C.byref(vd), off[0], off[1], off[2], counts.data_ptr(), None), "saf_volume_absorb")
    torch.cuda.synchronize()
    got = _grids(d_dev, d_n, kind)
    for name in want:
        assert np.array_equal(_np_bits(got[name]), _np_bits(want[name])), f"{name} differs from the restatement"
    # said once more without the restatement's help: outside the overlap and where the source's count is 0, every byte stands
    rows, tsdf = m["copy"] | m["blend"], m["t_copy"] | m["t_blend"]
    for name in got:
        keep = ~(tsdf if name in ("tsdf", "tsdf_weight") else rows)
        assert np.array_equal(_np_bits(got[name])[keep], _np_bits(before_d[name])[keep]), f"{name} was written where it must not be"
    # ... nothing poisoned was read ...
    assert np.isfinite(ref.widen(got["clip_feat"], kind)[rows]).all() and np.isfinite(got["rgb"][rows]).all()
    assert np.isfinite(got["tsdf"][tsdf]).all()
    if classes:
        assert (got["labels_one_hot"][rows] >= 0).all()
    assert counts.tolist() == [5 + inc[0], 7 + inc[1], 11 + inc[2], 13 + inc[3]], "the counters are added to, exactly"
    assert inc == (int(m["blend"].sum()), int(m["copy"].sum()), int(m["t_blend"].sum()), int(m["t_copy"].sum()))
    # ... and the source is only read
    for name, t in src.items():
        assert torch.equal(_bits(s_dev[name]).cpu(), _bits(t)), f"the source's {name} changed"


# ---- (b) offsets beyond 2^31 elements and 4 GB --------------------------------------------------------------------------------
def test_pass_addresses_rows_beyond_4_gigabytes():
    dim, s_n, d_n = 8192, (64, 64, 65), (64, 64, 66)
    ns, nd = int(np.prod(s_n)), int(np.prod(d_n))
    assert ns * dim > 1 << 31 and ns * dim * 2 > 1 << 32
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5)
    last = torch.arange(ns - 100, ns, device=dev)
    x, y, z = last // (s_n[1] * s_n[2]), (last // s_n[2]) % s_n[1], last % s_n[2]
    there = (x * d_n[1] + y) * d_n[2] + z  # the same voxels in the destination's numbering
    assert int(there.min()) * dim * 2 > 1 << 32
    zeros = lambda n, *shape, dtype=torch.float32: torch.zeros((n,) + shape, dtype=dtype, device=dev)
    src = {"tsdf": zeros(ns), "tsdf_weight": zeros(ns, dtype=torch.int32), "weight": zeros(ns, dtype=torch.int32), "rgb": zeros(ns, 3),
           "clip_feat": torch.empty((ns, dim), dtype=torch.bfloat16, device=dev)}  # (untouched rows: whatever the allocator left)
    dst = {"tsdf": zeros(nd), "tsdf_weight": zeros(nd, dtype=torch.int32), "weight": zeros(nd, dtype=torch.int32), "rgb": zeros(nd, 3),
           "clip_feat": zeros(nd, dim, dtype=torch.bfloat16)}
    ws = torch.arange(1, 101, dtype=torch.int32, device=dev)
    wd = torch.where(torch.arange(100, device=dev) % 2 == 0, torch.arange(3, 103, dtype=torch.int32, device=dev), 0).int()  # half blended
    src["weight"][last] = ws
    dst["weight"][there] = wd
    rows_s = torch.randn((100, dim), generator=g, device=dev).to(torch.bfloat16)
    rows_d = torch.randn((100, dim), generator=g, device=dev).to(torch.bfloat16)
    src["clip_feat"][last] = rows_s
    dst["clip_feat"][there[wd > 0]] = rows_d[wd > 0]
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    vs, vd = _descriptor(src, s_n, dim, _abi.SAF_BF16), _descriptor(dst, d_n, dim, _abi.SAF_BF16)
    check(lib().saf_volume_absorb(C.byref(vs), C.byref(vd), 0, 0, 0, counts.data_ptr(), None), "saf_volume_absorb")
    torch.cuda.synchronize()
    # the restatement's own pieces on the hundred rows
    ws_h, wd_h = ws.cpu().numpy(), wd.cpu().numpy()
    blend = wd_h > 0
    cs, cd, w = ref.coefficients(ws_h[blend], wd_h[blend])
    want = rows_s.cpu().view(torch.int16).numpy().copy()
    want[blend] = ref.narrow(ref.mix(ref.widen(want[blend], "bf16"), ref.widen(rows_d.cpu().view(torch.int16).numpy()[blend], "bf16"),
                                     cs[:, None], cd[:, None]), "bf16")
    got = dst["clip_feat"].index_select(0, there).cpu().view(torch.int16).numpy()
    assert np.array_equal(got, want)
    want_w = ws_h.copy()
    want_w[blend] = w
    assert np.array_equal(dst["weight"][there].cpu().numpy(), want_w) and int(dst["weight"].sum()) == int(want_w.sum())
    assert counts.tolist() == [50, 50, 0, 0]
    assert torch.equal(src["clip_feat"].index_select(0, last).view(torch.int16), rows_s.view(torch.int16)), "the source changed"
    untouched = torch.ones(nd, dtype=torch.bool, device=dev)
    untouched[there] = False
    sample = torch.cat((torch.arange(0, nd, 997, device=dev), torch.arange(nd - 300, nd, device=dev)))
    sample = sample[untouched[sample]]
    assert sample.numel() > 400 and int(_bits(dst["clip_feat"].index_select(0, sample)).abs().max()) == 0, "an untouched row was written"


# ---- (c) - (g): modules -------------------------------------------------------------------------------------------------------
UNION = ((-3, 0, -4), (32, 28, 36))  # the box around BOX_A and BOX_B, sizes rounded up to a multiple of 4 at the high end


def _snapshot(fz, seem=True):
    """The module's volume as it reads (queued frames fused, a deferred clear paid), cloned."""
    return {name: getattr(fz, name).clone() for name in _names(seem)}


def _raw(fz, seem=True):
    """The module's buffers as they are, cloned: nothing is brought up to date, a deferred clear stays owed."""
    return {name: fz._buffers[name].clone() for name in _names(seem)}


def _crop(t, box, into, fill=0):
    """A module's flat buffer ``t`` over ``box`` as a buffer over the box ``into``: ``fill`` where ``box`` has no voxel, and what
    falls outside ``into`` is dropped."""
    lo = tuple(max(b, i) for b, i in zip(box[0], into[0]))
    hi = tuple(min(b + n, i + k) for b, n, i, k in zip(box[0], box[1], into[0], into[1]))
    out = torch.full(tuple(into[1]) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    src = t.view(*box[1], *t.shape[1:])[tuple(slice(l - b, h - b) for l, h, b in zip(lo, hi, box[0]))]
    out[tuple(slice(l - i, h - i) for l, h, i in zip(lo, hi, into[0]))] = src
    return out.view(-1, *t.shape[1:])


def _side(name):
    return "tsdf_weight" if name in ("tsdf", "tsdf_weight") else "weight"


@pytest.mark.parametrize("seem", [pytest.param(True, id="ClipSeemFusion"), pytest.param(False, id="ClipFusion")])
def test_a_single_frame_volume_absorbed_is_that_frame_fused(seem):
    dim, m = 64, 6
    scan = _scan(dim, 11)
    fr = scan.frames
    a = _fuse(_module(scan, BOX_A, seem), fr[:m], seem)
    b = _fuse(_module(scan, BOX_A, seem), fr[m:m + 1], seem)
    full = _fuse(_module(scan, BOX_A, seem), fr[:m + 1], seem)
    b_before = _snapshot(b, seem)
    out = a.absorb(b)
    assert out.move is None and (out.index_offset, out.nvox) == BOX_A and out.overlap_nvox == BOX_A[1]
    for fz in (a, b, full):
        assert fz.stats()["window_rows"] == 0, "not the per-frame pipeline"
    assert int(out.rows_blended) > 100 and int(out.rows_copied) > 100 and int(out.rows_outside) == 0 and int(out.tsdf_outside) == 0
    for name in _names(seem):
        got, want = getattr(a, name), getattr(full, name)
        if name == "tsdf":  # the forward sweep's hardware reciprocal against the pass's IEEE division
            assert float((got - want).abs().max()) <= 1e-4, "tsdf"
        else:  # values, not bit patterns: a -0 sample that the first update stores as +0 is the one legitimate difference
            assert torch.equal(got, want), f"{name}: the absorbed frame is not the fused frame"
        assert torch.equal(_bits(getattr(b, name)), _bits(b_before[name])), f"the absorbed volume's {name} changed"


def _joined(dim, m, n, seem, fdt, grow=True):
    """A: frames 1..m over BOX_A; B: frames m+1..n over BOX_B; ``A.absorb(B)``.  Returns A, what A and B held before (raw buffers),
    B, and the record."""
    scan = _scan(dim, n)
    fr = scan.frames
    a = _fuse(_module(scan, BOX_A, seem, fdt), fr[:m], seem)
    b = _fuse(_module(scan, BOX_B, seem, fdt), fr[m:n], seem)
    a_before, b_before = _snapshot(a, seem), _snapshot(b, seem)
    out = a.absorb(b, grow=grow)
    for name in _names(seem):
        assert torch.equal(_bits(b._buffers[name]), _bits(b_before[name])), f"the absorbed volume's {name} changed"
    return a, a_before, b_before, b, out


def _touched_sets(a_before, b_before, into):
    """Per side, over the box ``into``: voxels both touched, only A, only B (boolean, flat)."""
    sets = {}
    for side in ("weight", "tsdf_weight"):
        wa = _crop(a_before[side], BOX_A, into) > 0
        wb = _crop(b_before[side], BOX_B, into) > 0
        sets[side] = (wa & wb, wa & ~wb, ~wa & wb)
    return sets


@pytest.mark.parametrize("seem", [pytest.param(True, id="ClipSeemFusion"), pytest.param(False, id="ClipFusion")])
def test_two_scans_joined_are_the_scan_fused_in_one(seem):
    dim, m, n = 64, 6, 11
    a, a_before, b_before, b, out = _joined(dim, m, n, seem, torch.float32)
    assert (out.index_offset, out.nvox) == UNION == (a.index_offset, tuple(int(v) for v in a.nvox))
    assert (out.other_index_offset, out.other_nvox) == BOX_B and out.move is not None and (out.move.old_index_offset, out.move.old_nvox) == BOX_A
    assert (out.overlap_in_self, out.overlap_in_other, out.overlap_nvox) == ((0, 2, 0), (0, 0, 0), BOX_B[1])
    scan = _scan(dim, n)
    full = _fuse(_module(scan, UNION, seem), scan.frames[:n], seem)
    sets = _touched_sets(a_before, b_before, UNION)
    both, only_a, only_b = sets["weight"]
    assert int(both.sum()) > 500 and int(only_a.sum()) > 50 and int(only_b.sum()) > 100, [int(s.sum()) for s in sets["weight"]]
    t_both, _, t_only_b = sets["tsdf_weight"]
    assert out.rows_blended.is_cuda and out.rows_blended.dtype == torch.int64 and out.rows_blended.dim() == 0
    assert [int(out.rows_blended), int(out.rows_copied), int(out.tsdf_blended), int(out.tsdf_copied)] == \
        [int(both.sum()), int(only_b.sum()), int(t_both.sum()), int(t_only_b.sum())]
    assert int(out.rows_outside) == 0 and int(out.tsdf_outside) == 0, "the grown box holds all of the other volume"
    for name in _names(seem):
        got, want = getattr(a, name), getattr(full, name)
        s_both, s_a, s_b = sets[_side(name)]
        if name in ("weight", "tsdf_weight", "labels_one_hot"):
            assert torch.equal(got[s_both], want[s_both]), f"{name}: counts where both saw the voxel"
        elif name == "clip_feat":
            _feat_close(got[s_both], want[s_both], 1e-4, "clip_feat where both saw the voxel")
        else:
            assert float((got[s_both] - want[s_both]).abs().max()) <= 1e-4, f"{name} where both saw the voxel"
        from_a, from_b = _crop(a_before[name], BOX_A, UNION), _crop(b_before[name], BOX_B, UNION)
        assert torch.equal(_bits(got)[s_a], _bits(from_a)[s_a]), f"{name}: a voxel only the first scan touched is not the first scan's"
        assert torch.equal(_bits(got)[s_b], _bits(from_b)[s_b]), f"{name}: a voxel only the second scan touched is not the second's"
        neither = ~(s_both | s_a | s_b)
        assert int(_bits(got)[neither].abs().max()) == 0, f"{name}: a voxel neither touched is not empty"


def test_two_scans_joined_without_growing_take_the_overlap_only():
    dim, m, n = 64, 6, 11
    grown, _, _, _, _ = _joined(dim, m, n, True, torch.float32)
    a, a_before, b_before, b, out = _joined(dim, m, n, True, torch.float32, grow=False)
    assert out.move is None and (out.index_offset, out.nvox) == BOX_A == (a.index_offset, tuple(int(v) for v in a.nvox))
    assert (out.overlap_in_self, out.overlap_in_other, out.overlap_nvox) == ((0, 2, 0), (3, 0, 4), (24, 18, 28))
    sets = _touched_sets(a_before, b_before, BOX_A)
    n_b = int((b_before["weight"] > 0).sum())
    taken = int(sets["weight"][0].sum()) + int(sets["weight"][2].sum())
    assert int(out.rows_blended) + int(out.rows_copied) == taken and int(out.rows_outside) == n_b - taken > 100
    t_taken = int(sets["tsdf_weight"][0].sum()) + int(sets["tsdf_weight"][2].sum())
    assert int(out.tsdf_outside) == int((b_before["tsdf_weight"] > 0).sum()) - t_taken > 0
    in_b = _crop(torch.ones(int(np.prod(BOX_B[1])), dtype=torch.bool, device="cuda"), BOX_B, BOX_A, fill=False)
    assert int((~in_b).sum()) > 0
    for name in NAMES:
        got = getattr(a, name)
        assert torch.equal(_bits(got)[~in_b], _bits(a_before[name])[~in_b]), f"{name}: outside the overlap the volume is not what it was"
        same = _crop(getattr(grown, name), UNION, BOX_A)  # the same arithmetic on the same voxels
        assert torch.equal(_bits(got)[in_b], _bits(same)[in_b]), f"{name}: inside the overlap, against the grown volume"


# ---- (e) 16-bit modules against the restatement on their own buffers ----------------------------------------------------------
@pytest.mark.parametrize("fdt", [pytest.param(torch.bfloat16, id="bf16"), pytest.param(torch.float16, id="fp16")])
def test_16_bit_modules_joined_equal_the_restatement_bit_for_bit(fdt):
    dim, m, n = 64, 6, 11
    kind = KIND_OF[fdt]
    a, a_before, b_before, b, out = _joined(dim, m, n, True, fdt)
    assert a.clip_feat.dtype == fdt and int(out.rows_blended) > 500 and int(out.rows_copied) > 100
    off = tuple(u - o for u, o in zip(UNION[0], BOX_B[0]))
    moved = {name: _crop(t, BOX_A, UNION) for name, t in a_before.items()}  # move_grid is a copy into zeros (test_carry_gpu.py)
    want, inc = ref.absorb(_grids(b_before, BOX_B[1], kind), _grids(moved, UNION[1], kind), off, kind)
    got = _grids(_snapshot(a), UNION[1], kind)
    for name in NAMES:
        assert np.array_equal(_np_bits(got[name]), _np_bits(want[name])), f"{name} differs from the restatement"
    assert inc == (int(out.rows_blended), int(out.rows_copied), int(out.tsdf_blended), int(out.tsdf_copied))


# ---- (f) stale rows -----------------------------------------------------------------------------------------------------------
def _stale(scan, box, frames):
    """A module whose deferred clear is still owed: rows of NaN left by a first scan, a lazy reset, ``frames`` through the windowed
    path (which never reads a weight-0 row)."""
    fz = _fuse(_module(scan, box), scan.frames[:24])
    fz._buffers["clip_feat"].fill_(float("nan"))  # whatever the first scan left must never be seen again
    fz.reset()
    _fuse(fz, frames)
    assert fz._feat_stale and bool(torch.isnan(fz._buffers["clip_feat"]).any())
    return fz


def test_absorb_with_rows_that_are_still_stale_on_either_side(rows_form):
    dim = 256
    scan = _scan(dim, 64)
    fr = scan.frames
    mine, theirs = fr[16:40], fr[40:64]  # (24 frames each: the windowed path)
    other = _fuse(_module(scan, BOX_B), theirs)
    twin = _fuse(_module(scan, BOX_A), mine)
    twin.absorb(other)
    assert twin.stats()["window_rows"] > 0 and other.stats()["window_rows"] > 0, "the windowed path did not run"
    want = _snapshot(twin)
    assert int((want["weight"] > 0).sum()) > 500
    for stale_self, stale_other in ((True, False), (False, True), (True, True)):
        fz = _stale(scan, BOX_A, mine) if stale_self else _fuse(_module(scan, BOX_A), mine)
        ot = _stale(scan, BOX_B, theirs) if stale_other else other
        out = fz.absorb(ot)
        assert fz._feat_stale, "the grown volume's clear stays owed"
        if stale_other:
            assert ot._feat_stale and bool(torch.isnan(ot._buffers["clip_feat"]).any()), "the other volume's clear was paid"
        assert int(out.rows_blended) > 0 and int(out.rows_copied) > 0
        for name in NAMES:
            assert torch.equal(_bits(getattr(fz, name)), _bits(want[name])), f"{name} differs from the absorb into a cleared twin"
        assert int(_bits(fz.clip_feat)[fz.weight == 0].abs().max()) == 0, "a row of an untouched voxel does not read as zero"
        assert int(fz.labels_one_hot[fz.weight == 0].abs().max()) == 0
    # without growing: this volume's own stale rows stay where they are, owed
    fz = _stale(scan, BOX_A, mine)
    twin = _fuse(_module(scan, BOX_A), mine)
    fz.absorb(other, grow=False)
    twin.absorb(other, grow=False)
    assert fz._feat_stale and bool(torch.isnan(fz._buffers["clip_feat"]).any())
    for name in NAMES:
        assert torch.equal(_bits(getattr(fz, name)), _bits(getattr(twin, name))), f"{name}: grow=False, against a cleared twin"
    assert int(_bits(fz.clip_feat)[fz.weight == 0].abs().max()) == 0


# ---- (g) behind the queues ----------------------------------------------------------------------------------------------------
def test_absorb_behind_the_queues_of_one_frame_calls(rows_form):
    dim, m, n = 256, 40, 50
    scan = _scan(dim, 64)
    fr = scan.frames
    fz, other = _module(scan, BOX_A, defer=True), _module(scan, BOX_B, defer=True, first_frame=m)
    _one_by_one(fz, fr[:m])
    _one_by_one(other, fr[m:n])
    q = fz.__dict__["_queue"]
    assert fz.pending_frames + q.ring.sess_frames == m and fz.pending_frames > 0 and fz._queue_busy(), "the calls did not go through the queue"
    assert other.pending_frames == n - m and other._queue_busy()
    out = fz.absorb(other)
    assert not fz._queue_busy() and fz.pending_frames == 0 and not other._queue_busy() and other.pending_frames == 0
    assert fz.clip.calls == m and other.clip.calls == n
    # the flushed case
    fz2, other2 = _module(scan, BOX_A, defer=True), _module(scan, BOX_B, defer=True, first_frame=m)
    _one_by_one(fz2, fr[:m])
    _one_by_one(other2, fr[m:n])
    fz2.flush()
    other2.flush()
    torch.cuda.synchronize()
    out2 = fz2.absorb(other2)
    assert int(out.rows_blended) == int(out2.rows_blended) > 0 and int(out.rows_copied) == int(out2.rows_copied) > 0
    for name in NAMES:
        assert torch.equal(_bits(getattr(fz, name)), _bits(getattr(fz2, name))), f"{name} differs from the flushed case"
        assert torch.equal(_bits(getattr(other, name)), _bits(getattr(other2, name))), f"the other volume's {name}"
    # the module afterwards: frames, a view, a mesh, a move
    fz.clip.calls = fz.segmentation_model.calls = n
    _one_by_one(fz, fr[n:n + 4])
    assert fz.pending_frames > 0, "the calls after the absorb did not go through the queue"
    view = fz.render(fr[0]["pose"][0].cuda(), fr[0]["K"][0].cuda(), H, W)
    assert int(view.hit.sum()) > 0 and int(view.voxel.max()) < fz.weight.numel() and fz.pending_frames == 0
    assert fz.stats()["frames"] == m + 4
    assert not hasattr(fz, "voxel_obj_idx") and not hasattr(fz, "objects_segmentation_color")
    fz.voxel_obj_idx = torch.full((fz.weight.numel(),), -1, dtype=torch.int32, device="cuda")
    fz.objects_segmentation_color = fz.rgb.clone()
    verts, faces = fz.extract_mesh()[:2]
    assert len(faces) > 100 and len(verts) > 100
    w_before = int((fz.weight > 0).sum())
    move = fz.move_grid(*BOX_B)
    assert 0 < int(move.rows_carried) <= w_before and int((fz.weight > 0).sum()) == int(move.rows_carried)
    assert (fz.index_offset, tuple(int(v) for v in fz.nvox)) == BOX_B
