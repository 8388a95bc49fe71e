"""CPU: the object layer's bookkeeping against the reference's own results (tests/golden/object_bookkeeping.json, written by
tools/gen_golden_objects.py), ``object_slots``, the host-side argument checks of saf_object_stats, and the arithmetic its
determinism rests on."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from host_stubs import fake_volume
from spatially_aware_ai_amd import _abi, _lib

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "object_bookkeeping.json")


class _Model:
    def __init__(self, labels):
        self.labels = list(labels)
        self.model_trained = False


def _plain(knowledge):
    """scene_knowledge as JSON holds it (voxel tuples become lists)."""
    return json.loads(json.dumps(knowledge, default=lambda a: a.tolist()))


def test_merge_and_mark_match_the_reference():
    from spatially_aware_ai_amd.objects import mark_object_of_interest, merge_objects

    rec = json.load(open(GOLDEN))
    knowledge = copy.deepcopy(rec["scene_knowledge"])
    model = _Model(rec["labels"])
    ops = [s["op"] for s in rec["steps"]]
    assert ops.count("merge_objects") >= 4 and ops.count("mark_object_of_interest") >= 2
    for step in rec["steps"]:
        if step["op"] == "merge_objects":
            ret = merge_objects(knowledge, None, model, list(step["merge_list"]), step["new_label"])
            if len(step["merge_list"]) == 0:
                assert ret is knowledge and step["new_id"] is None  # the reference returns the dictionary alone
            else:
                new_id, knowledge = ret
                assert new_id == step["new_id"]
        else:
            knowledge = mark_object_of_interest(knowledge, model, list(step["object_list"]))
        assert model.labels == step["labels"], step["op"]
        got, want = _plain(knowledge), step["scene_knowledge"]
        assert list(got["unique_objects"]) == list(want["unique_objects"])  # insertion order is part of the data model
        assert list(got["object_counts"].items()) == list(want["object_counts"].items())
        assert got == want, step["op"]
    # what the steps were chosen to show
    s0, s1, s2 = rec["steps"][:3]
    assert s0["new_id"].endswith("-merged:1") and s0["scene_knowledge"]["unique_objects"][s0["new_id"]]["merged"] is True
    assert s1["scene_knowledge"]["unique_objects"][s1["new_id"]]["merged"] is False
    assert ":" in s2["new_label"] and s2["new_id"] != s2["new_label"] and s2["new_id"].split(":")[0] == s2["new_label"].split(":")[0]
    for s in (s0, s1, s2):
        assert s["scene_knowledge"]["unique_objects"][s["new_id"]]["object_index"] == s["labels"].index(s["new_id"])


def test_merge_joins_array_voxel_lists_and_relabels_a_grid():
    from spatially_aware_ai_amd.io import ArrayList
    from spatially_aware_ai_amd.objects import merge_objects

    obj = lambda idx, vox: {"class_id": 1, "class_label": "a", "voxels": ArrayList(np.array(vox), tuples=True), "object_index": idx,
                            "gt_label": "x", "user_modified": False, "merged": False, "removed": False, "color": None}
    know = {"unique_objects": {"a:1": obj(-2, [[0, 0, 0], [0, 0, 1]]), "a:2": obj(-3, [[1, 1, 1]]), "a:3": obj(-4, [[2, 2, 2]])},
            "object_counts": {"a": 3}}
    grid = torch.tensor([-2, -2, -1, -3, -4, 7], dtype=torch.int32)
    model = _Model(["null", "kept"])
    new_id, know = merge_objects(know, None, model, ["a:1", "a:2"], "pair", voxel_obj_idx=grid)
    assert new_id == "pair-merged:1" and model.labels == ["null", "kept", "pair-merged:1"]
    assert know["unique_objects"][new_id]["voxels"] == [(0, 0, 0), (0, 0, 1), (1, 1, 1)]
    assert grid.tolist() == [2, 2, -1, 2, -4, 7]


def test_object_slots():
    from spatially_aware_ai_amd.objects import object_slots

    know = {"unique_objects": {
        "chair:1": {"object_index": -2, "removed": False},
        "gone:1": {"object_index": -3, "removed": True},
        "my mug:1": {"object_index": 4, "removed": False},
        "sofa:1": {"object_index": -5},
        "lamp:1": {"object_index": 1, "removed": False},
    }}
    grid = torch.tensor([[[-1, -2, -3], [4, -5, 1]], [[0, 2, -4], [-2, 4, 133]]], dtype=torch.int32)
    slot, ids = object_slots(grid, know)
    assert ids == ["chair:1", "my mug:1", "sofa:1", "lamp:1"]
    assert slot.dtype == torch.int32 and slot.shape == (12,)
    assert slot.tolist() == [-1, 0, -1, 1, 2, 3, -1, -1, -1, 0, 1, -1]
    # int64 grids (torch.where in discover_objects keeps int32; callers may hold either) give the same answer
    assert torch.equal(object_slots(grid.long(), know)[0], slot)
    slot0, ids0 = object_slots(grid, {"unique_objects": {"gone:1": {"object_index": -3, "removed": True}}})
    assert ids0 == [] and slot0.tolist() == [-1] * 12
    know["unique_objects"]["twin:1"] = {"object_index": 4, "removed": False}
    with pytest.raises(ValueError, match="share an object_index"):
        object_slots(grid, know)
    know["unique_objects"]["twin:1"]["removed"] = True  # a removed twin does not count
    assert object_slots(grid, know)[1] == ids


def _fake_volume(dtype=_abi.SAF_F32):
    return fake_volume(n=8, dim=16, dtype=dtype)


def test_object_stats_rejects_bad_arguments_on_the_host():
    l = _lib.lib()
    assert l.saf_abi_version() == 7 == _abi.ABI_VERSION
    P = 4096  # a non-NULL, 256-byte aligned stand-in: every call below returns before anything is launched
    call = lambda vol, slot=P, k=3, norm=_abi.SAF_NORM_L2, count=P, bbox=P, ws=P, wsb=1 << 20: l.saf_object_stats(
        ctypes.byref(vol) if vol is not None else None, slot, k, norm, count, None, None, bbox, None, None, P, ws, wsb, None)
    zero = _abi.SafVolume()  # all zeros
    assert call(zero) == _abi.SAF_E_INVALID and b"bad volume" in l.saf_last_error()
    good = _fake_volume()
    assert call(None) == _abi.SAF_E_INVALID
    assert call(good, slot=None) == _abi.SAF_E_INVALID
    assert call(good, count=None) == _abi.SAF_E_INVALID
    assert call(good, bbox=None) == _abi.SAF_E_INVALID
    assert call(good, k=0) == _abi.SAF_E_INVALID and call(good, k=-2) == _abi.SAF_E_INVALID
    big = _fake_volume()
    big.nx, big.ny, big.nz = 2048, 1024, 1024  # 2^31 voxels
    assert call(big, wsb=1 << 40) == _abi.SAF_E_INVALID
    need = l.saf_object_stats_workspace_bytes(8 ** 3, 3, 16)
    assert need >= 3 * (8 * (9 + 16) + 24) and need % 256 == 0
    assert call(good, wsb=need - 1) == _abi.SAF_E_INVALID and b"workspace" in l.saf_last_error()
    assert call(good, ws=None, wsb=need) == _abi.SAF_E_INVALID
    assert call(good, ws=P + 8, wsb=need) == _abi.SAF_E_INVALID  # misaligned
    assert call(good, norm=_abi.SAF_NORM_NONE) == _abi.SAF_E_UNSUPPORTED and b"SAF_NORM_NONE" in l.saf_last_error()
    assert call(good, norm=7) == _abi.SAF_E_INVALID
    assert call(_fake_volume(dtype=_abi.SAF_F16)) == _abi.SAF_E_UNSUPPORTED


def test_object_stats_workspace_bytes():
    l = _lib.lib()
    size = l.saf_object_stats_workspace_bytes
    assert size(0, 3, 16) == 0 and size(-5, 3, 16) == 0 and size(1 << 31, 3, 16) == 0
    assert size(512, 0, 16) == 0 and size(512, -1, 16) == 0 and size(512, 3, 0) == 0
    assert size((1 << 31) - 1, 1, 1) > 0
    # the accumulators: per object 9 + D 64-bit words and a box of six 32-bit ones
    assert size(256 ** 3, 3000, 512) >= 3000 * (8 * (9 + 512) + 24)
    assert size(256 ** 3, 3000, 512) < 3000 * (8 * (9 + 512) + 24) + 256


def test_fixed_point_sum_does_not_depend_on_the_order():
    """The contract's arithmetic restated in NumPy: terms v in [-1, 1] enter as rint(v 2^30) in 64-bit integers.  Any order of
    summation -- any split into partial sums, as the kernel's chunks and atomics produce -- gives the same integer, hence the same
    f32 mean; a float sum of the same terms does depend on the order."""
    rng = np.random.default_rng(7)
    n, d = 20000, 8
    f = rng.standard_normal((n, d)).astype(np.float32) * rng.choice([1e-3, 1.0, 1e4], (n, 1)).astype(np.float32)
    v = f / np.sqrt((f * f).sum(1, dtype=np.float32))[:, None]
    q = np.rint(v * np.float32(2.0 ** 30)).astype(np.int64)
    assert np.abs(q).max() <= 2 ** 30
    mean = lambda s: (s.astype(np.float64) / (2.0 ** 30 * n)).astype(np.float32)
    want = q.sum(0)
    float_sums = set()
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(n)
        parts = np.array_split(q[perm], 37 + seed)  # chunks, each summed on its own, then added in another order again
        got = sum((p.sum(0) for p in reversed(parts)), np.zeros(d, np.int64))
        assert np.array_equal(got, want)
        assert mean(got).tobytes() == mean(want).tobytes()
        float_sums.add(np.add.reduce(v[perm], axis=0, dtype=np.float32).tobytes())
    assert len(float_sums) > 1, "the float sum was expected to depend on the order"
    # the quantisation costs at most 2^-31 per term, so the mean is within 2^-31 of the exact mean of v
    exact = v.astype(np.float64).mean(0)
    assert np.abs(want.astype(np.float64) / (2.0 ** 30 * n) - exact).max() <= 2.0 ** -31
    # and the bound the header states: 2^31 members of magnitude 2^30 stay below 2^63
    assert (2 ** 31) * (2 ** 30) < 2 ** 63
