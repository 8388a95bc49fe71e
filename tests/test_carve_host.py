"""Host: free-space carving's parts that need no GPU (spatially_aware_ai_amd/_carve.py, include/saf.h: saf_free_space_observe,
saf_volume_carve) -- the erosion of the depth against a hand-written loop, the restated decision at its boundaries, the
refusals of the Python surface and of the two entries, the synthetic scene's defaults, and that no case of the GPU tests is
vacuous (the oracle classifies on the CPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi, _carve, clipfusion
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd._lib import SafError, lib

import carve_cases as cc
import carve_reference as ref
from host_stubs import P, fake_volume


# ---- erode --------------------------------------------------------------------------------------------------------------------
def _erode_by_hand(d, e):
    h, w = d.shape
    out = np.zeros_like(d)
    for y in range(h):
        for x in range(w):
            window = [d[yy, xx] for yy in range(max(y - e, 0), min(y + e, h - 1) + 1) for xx in range(max(x - e, 0), min(x + e, w - 1) + 1)]
            if all(np.isfinite(v) and v > 0 for v in window):
                out[y, x] = min(window)
    return out


def _image():
    """8 x 6 (W x H) with a hole, a NaN, an inf, a negative value; the borders are ordinary pixels with clipped windows."""
    rng = np.random.default_rng(3)
    d = (rng.random((6, 8)) * 2 + 1).astype(np.float32)
    d[2, 3] = 0.0
    d[0, 7] = np.nan
    d[5, 0] = np.inf
    d[4, 6] = -1.5
    return d


@pytest.mark.parametrize("e", [0, 1, 2])
def test_erode_is_the_clipped_window_minimum_or_missing(e):
    d = _image()
    want = d.copy() if e == 0 else _erode_by_hand(d, e)
    got = _carve.erode_depth(torch.from_numpy(d)[None], e)[0].numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "erode_depth"
    assert np.array_equal(ref.erode(d, e).view(np.int32), want.view(np.int32)), "the restatement's erode"
    if e == 1:
        assert want[0, 0] == d[:2, :2].min() and want[5, 7] == 0.0 == want[1, 2] and want[3, 3] == 0.0  # border; -1.5; the hole
        assert (want > 0).sum() >= 10 and (want == 0).sum() >= 20
    # a batch is eroded image by image
    two = torch.from_numpy(np.stack((d, d[::-1].copy())))
    got2 = _carve.erode_depth(two, e).numpy()
    assert np.array_equal(got2[1].view(np.int32), (d[::-1] if e == 0 else _erode_by_hand(d[::-1].copy(), e)).view(np.int32))


def test_erode_refuses_what_is_not_a_count():
    for bad in (-1, 1.0, True, None):
        with pytest.raises(SafError, match="erode"):
            _carve.erode_depth(torch.ones(1, 4, 4), bad)


# ---- the decision -------------------------------------------------------------------------------------------------------------
def test_decision_at_its_boundaries():
    #                 untouched  too few   just enough  supported at the bound  one too many  never seen
    weight = np.array([0, 3, 3, 3, 3, 1], dtype=np.int32)
    seen = np.array([9, 2, 3, 3, 3, 0], dtype=np.int32)
    hit = np.array([0, 0, 0, 1, 2, 0], dtype=np.int32)
    carved, counts = ref.decide(weight, seen, hit, min_views=3, max_support=1)
    assert carved.tolist() == [False, False, True, True, False, False]
    assert counts == [5, 2, 1, 1]
    carved, counts = ref.decide(weight, seen, hit, min_views=3, max_support=0)
    assert carved.tolist() == [False, False, True, False, False, False] and counts == [5, 1, 2, 1]
    carved, counts = ref.decide(weight, seen, hit, min_views=2, max_support=0)
    assert carved.tolist() == [False, True, True, False, False, False] and counts == [5, 2, 2, 0]
    bufs = {"weight": weight, "rgb": np.ones((6, 3), dtype=np.float32), "clip_feat": np.full((6, 4), 7, dtype=np.int16)}
    out = ref.carve(bufs, carved)
    assert out["weight"].tolist() == [0, 0, 0, 3, 3, 1] and out["rgb"].sum() == 12 and out["clip_feat"].sum() == 7 * 16
    assert bufs["weight"].tolist() == weight.tolist(), "the restatement works on a copy"


# ---- the Python surface's refusals ----------------------------------------------------------------------------------------------
class _Stub(clipfusion._FusionVolumeMixin):
    """A module's host state without buffers: every refusal below is decided before anything of the device is touched."""

    accum_mode = _abi.SAF_RUNNING_MEAN
    x_planes = None
    index_offset = (1, -2, 3)
    nvox = torch.tensor([4, 5, 6])


def _evidence(off=(1, -2, 3), nvox=(4, 5, 6), n=None, dtype=torch.int32):
    n = nvox[0] * nvox[1] * nvox[2] if n is None else n
    return _carve.FreeSpaceEvidence(torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype), 0, off, nvox)


def test_evidence_of_another_box_is_refused():
    s = _Stub()
    s._check_evidence("carve", _evidence())  # the module's own box
    for ev, what in ((_evidence(off=(0, 0, 0)), "belongs to the box"), (_evidence(nvox=(4, 5, 7)), "belongs to the box"),
                     (_evidence(n=7), "120 entries"), (_evidence(dtype=torch.int64), "int32")):
        with pytest.raises(SafError, match=what):
            s._check_evidence("carve", ev)
    with pytest.raises(SafError, match="FreeSpaceEvidence"):
        s._check_evidence("carve", (torch.zeros(120), torch.zeros(120)))
    for call in (lambda: s.carve(evidence=_evidence(off=(0, 0, 0))),
                 lambda: s.observe_free_space(torch.ones(1, 4, 4), torch.eye(4)[None], torch.eye(3)[None], evidence=_evidence(nvox=(6, 5, 4)))):
        with pytest.raises(SafError, match="belongs to the box"):
            call()


def test_unfit_modules_and_bad_knobs_are_refused():
    frames = (torch.ones(1, 4, 4), torch.eye(4)[None], torch.eye(3)[None])
    s = _Stub()
    s.x_planes = torch.arange(4)
    for call in (lambda: s.carve(evidence=_evidence()), lambda: s.observe_free_space(*frames)):
        with pytest.raises(SafError, match="x_planes"):
            call()
    s = _Stub()
    s._shard_stripes = [(0, 8)]
    with pytest.raises(SafError, match="stripes"):
        s.carve(evidence=_evidence())
    s = _Stub()
    s.__dict__["_poisoned"] = "a flush failed"
    with pytest.raises(SafError, match="a flush failed"):
        s.observe_free_space(*frames)
    s = _Stub()
    s.accum_mode = _abi.SAF_SUM
    for call in (lambda: s.carve(evidence=_evidence()), lambda: s.observe_free_space(*frames)):
        with pytest.raises(SafError, match="running means only"):
            call()
    s = _Stub()
    for kw, what in ((dict(min_views=0), "min_views"), (dict(min_views=True), "min_views"), (dict(min_views=2.0), "min_views"),
                     (dict(max_support=-1), "max_support"), (dict(), "give the evidence"),
                     (dict(depth_imgs=frames[0]), "come together")):
        with pytest.raises(SafError, match=what):
            s.carve(**kw)
    for args, what in (((torch.ones(4, 4), frames[1], frames[2]), r"\[B,H,W\]"), ((frames[0], torch.eye(4), frames[2]), "poses"),
                       ((frames[0], frames[1], torch.eye(3)[None].repeat(2, 1, 1)), "poses")):
        with pytest.raises(SafError, match=what):
            s.observe_free_space(*args)


# ---- the entries' refusals, decided on the host before anything is launched ------------------------------------------------------
def _observe(vol, depth=P, batch=2, height=48, width=64, poses=P, K=P, seen=P, hit=P):
    return lib().saf_free_space_observe(C.byref(vol) if vol is not None else None, depth, batch, height, width, poses, K, seen, hit, None)


def _carve_call(vol, seen=P, hit=P, min_views=2, max_support=0, carved=None, counts=None):
    return lib().saf_volume_carve(C.byref(vol) if vol is not None else None, seen, hit, min_views, max_support, carved, counts, None)


def _vol(**kw):
    kw.setdefault("trunc", 0.1)
    kw.setdefault("dim", 8)
    return fake_volume(**kw)


def test_observe_refuses_on_the_host():
    bad = [dict(vol=None), dict(vol=_vol(weight=None)), dict(vol=_vol(axis_y=None)), dict(depth=None), dict(poses=None), dict(K=None),
           dict(seen=None), dict(hit=None), dict(batch=0), dict(height=0), dict(width=-3), dict(vol=_vol(nx=0)), dict(vol=_vol(trunc=0.0)),
           dict(vol=_vol(nx=2048, ny=1024, nz=1024)), dict(height=1 << 16, width=1 << 15), dict(seen=P + 2), dict(depth=P + 1),
           dict(vol=_vol(weight=P + 2))]
    for kw in bad:
        kw.setdefault("vol", _vol())
        assert _observe(**kw) == _abi.SAF_E_INVALID, kw
    assert _observe(_vol(accum_mode=_abi.SAF_SUM)) == _abi.SAF_E_UNSUPPORTED
    assert b"running means only" in lib().saf_last_error()


def test_carve_refuses_on_the_host():
    bad = [dict(vol=None), dict(seen=None), dict(hit=None), dict(min_views=0), dict(min_views=-1), dict(max_support=-1),
           dict(vol=_vol(rgb=None)), dict(vol=_vol(clip_feat=None)), dict(vol=_vol(n_classes=3)), dict(vol=_vol(dim=0)), dict(vol=_vol(nz=0)),
           dict(vol=_vol(nx=2048, ny=1024, nz=1024)), dict(vol=_vol(dtype=7)), dict(hit=P + 2), dict(counts=P + 4),
           dict(vol=_vol(tsdf=P + 1)), dict(vol=_vol(clip_feat=P + 2)), dict(vol=_vol(dtype=_abi.SAF_BF16, clip_feat=P + 1)),
           dict(vol=_vol(n_classes=3, labels_one_hot=P + 2))]
    for kw in bad:
        kw.setdefault("vol", _vol())
        assert _carve_call(**kw) == _abi.SAF_E_INVALID, kw
    assert _carve_call(_vol(accum_mode=_abi.SAF_SUM)) == _abi.SAF_E_UNSUPPORTED


# ---- synthetic ------------------------------------------------------------------------------------------------------------------
def test_the_scene_defaults_are_what_they_were():
    kw = dict(width=64, height=48, feat_dim=8, npy=cc.NPY, npx=cc.NPX, depth_kind="B")
    plain = syn.make_frames(17, 3, **kw)
    stated = syn.make_frames(17, 3, sphere=((0.0, 0.0, 0.0), 0.9), **kw)
    for a, b in zip(plain, stated):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k].view(torch.int32) if a[k].is_floating_point() else a[k],
                               b[k].view(torch.int32) if b[k].is_floating_point() else b[k]), k
    # the sphere of the formula the scene always had, written out: |o + s d| = 0.9 in float64
    f = plain[0]
    pose, k = f["pose"][0].double(), f["K"][0].double()
    v, u = 24, 32  # the principal point's pixel: the ray through the origin's neighbourhood hits the sphere
    d = pose[:3, :3] @ torch.tensor([(u - k[0, 2]) / k[0, 0], (v - k[1, 2]) / k[1, 1], 1.0], dtype=torch.float64)
    o = pose[:3, 3]
    a_, b_, c_ = d @ d, 2 * (d @ o), o @ o - 0.9 ** 2
    s = (-b_ - (b_ * b_ - 4 * a_ * c_).sqrt()) / (2 * a_)
    assert abs(float(f["depth"][0, v, u]) - float(s)) < 1e-6
    # the same seed without the sphere, or with it elsewhere: the same cameras, rgb, feature and label maps, another depth
    empty = syn.make_frames(17, 3, sphere=None, **kw)
    moved = syn.make_frames(17, 3, sphere=cc.MOVED_TO, **kw)
    for a, b, c in zip(plain, empty, moved):
        for name in ("pose", "K", "rgb", "feat", "labels"):
            assert torch.equal(a[name], b[name]) and torch.equal(a[name], c[name]), name
        assert float(b["depth"].min()) > 1.2 and not torch.equal(a["depth"], b["depth"]) and not torch.equal(b["depth"], c["depth"])
        assert bool((c["depth"] <= b["depth"]).all()), "a sphere only ever hides the wall behind it"
    scan = syn.SyntheticScan(5, 2, 64, 48, 8)
    same = syn.SyntheticScan(5, 2, 64, 48, 8, sphere=syn.DEFAULT_SPHERE)
    gone = syn.SyntheticScan(5, 2, 64, 48, 8, sphere=None)
    for i in range(2):
        assert all(torch.equal(scan.frames[i][k], same.frames[i][k]) for k in scan.frames[i])
        assert not bool((gone.frames[i]["surface"] == 0).any()) and bool((scan.frames[i]["surface"] == 0).any())


# ---- the GPU tests' cases, on the CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_no_case_of_the_gpu_tests_is_vacuous(oracle, name):
    c = cc.CASES[name]
    weight, tsdf_weight = cc.oracle_weight(oracle, c)
    assert int(((weight == 0) & (tsdf_weight > 0)).sum()) >= 200, "voxels that only the TSDF side knows"
    settings = cc.KNOBS if name == cc.KNOB_CASE else [(c["min_views"], c["max_support"])]
    supported = few = 0
    for mv, ms in settings:
        seen, hit, carved, counts = cc.expectation(oracle, c, weight, min_views=mv, max_support=ms)
        assert counts[1] >= 200 and counts[0] - counts[1] >= 200, (name, mv, ms, counts)
        assert not seen[weight == 0].any() and not hit[weight == 0].any()
        supported, few = max(supported, counts[2]), max(few, counts[3])
    if name == cc.KNOB_CASE:
        assert supported > 0 and few > 0
