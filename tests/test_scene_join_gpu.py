"""GPU: two reconstructions of one lattice put together (``scene.join_scenes``): the second scan is reconstructed on the first one's
lattice (``reconstruct_scene(lattice_of=...)``), the first one's volume absorbs it (``absorb``; saf_volume_absorb), no frame goes
through the backbones twice, and what comes out is -- within the rounding of two partial means -- the volume of a module that
fused all the frames over the final box, with labels, objects and mesh that are those of that volume."""
import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import synthetic as syn

from test_brick_form import _feat_close
from test_scene_extend_gpu import DIM, H, N_ALL, N_OLD, NAMES, W, _Part, _bits

pytestmark = pytest.mark.gpu


def _scan():
    scan = syn.SyntheticScan(23, N_ALL, W, H, DIM)
    for f in scan.frames[N_OLD:]:  # the second session stands half a metre further along x and y (tests/test_scene_extend_gpu.py)
        f["pose"] = f["pose"].clone()
        f["pose"][0, :3, 3] += torch.tensor([0.5, -0.4, 0.0])
    return scan


def _crop(t, box, into, fill=0):
    """A flat buffer over ``box`` as one over the box ``into``: ``fill`` where ``box`` has no voxel, the rest dropped."""
    lo = tuple(max(b, i) for b, i in zip(box[0], into[0]))
    hi = tuple(min(b + n, i + k) for b, n, i, k in zip(box[0], box[1], into[0], into[1]))
    out = torch.full(tuple(into[1]) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    src = t.reshape(*box[1], *t.shape[1:])[tuple(slice(l - b, h - b) for l, h, b in zip(lo, hi, box[0]))]
    out[tuple(slice(l - i, h - i) for l, h, i in zip(lo, hi, into[0]))] = src
    return out.view(-1, *t.shape[1:])


def _box(fz):
    return fz.index_offset, tuple(int(v) for v in fz.nvox)


def test_join_scenes_absorbs_the_second_reconstruction_and_runs_the_later_stages(rows_form):
    from spatially_aware_ai_amd.clip_seem_fusion import ClipSeemFusion, discover_objects
    from spatially_aware_ai_amd.clipfusion import lattice_box
    from spatially_aware_ai_amd.scene import join_scenes, reconstruct_scene

    scan = _scan()
    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    clip, seg = syn.ReplayClip(scan, class_names=names), syn.ReplaySeg(scan)
    config = {"voxel_size": 0.08, "trunc_vox": 3, "clip_patch_size": scan.patch, "clip_patch_stride": scan.stride}
    first = reconstruct_scene(_Part(scan, 0, N_OLD), config, clip, seg, names, colors)
    second = reconstruct_scene(_Part(scan, N_OLD, N_ALL), config, clip, seg, names, colors, lattice_of=first)
    assert clip.calls == N_ALL and seg.calls == N_ALL
    fz, other = first.fusion, second.fusion
    box_1, box_2 = _box(fz), _box(other)
    assert torch.equal(torch.as_tensor(other.origin), torch.as_tensor(fz.origin)) and second.scene_knowledge["scan_version"] == 0
    assert box_2 == lattice_box(fz, second.xyz, union=False) and box_2[0] != (0, 0, 0), "the second scan's own box on the first's lattice"
    before_1 = {name: getattr(fz, name).clone() for name in NAMES}
    before_2 = {name: getattr(other, name).clone() for name in NAMES}
    res = join_scenes(first, second, names, colors)
    assert clip.calls == N_ALL and seg.calls == N_ALL, "a frame went through the backbones again"
    assert res.fusion is fz and res.scene_knowledge["scan_version"] == 1 and res.object_matches is None
    for k in ("absorb", "label_argmax", "objects", "extract_mesh", "object_meshes"):
        assert res.seconds[k] > 0, k
    assert tuple(res.xyz.shape)[0] == tuple(first.xyz.shape)[0] + tuple(second.xyz.shape)[0]
    box = _box(fz)
    assert torch.equal(torch.as_tensor(res.nvox), fz.nvox) and all(v % 4 == 0 for v in box[1])
    for b in (box_1, box_2):
        assert all(o >= u and o + n <= u + k for o, n, u, k in zip(b[0], b[1], box[0], box[1])), "a scan's box is not inside the joined one"
    assert box != box_1, "the volume did not grow: the test means nothing"
    for name in NAMES:
        assert torch.equal(_bits(getattr(other, name)), _bits(before_2[name])), f"the second reconstruction's {name} changed"

    # ---- the volume: a fresh module over the final box, fed all 48 frames one after the other
    full = ClipSeemFusion(first.origin, 0.08, torch.tensor(box[1]), 3 * 0.08, False, scan.patch, scan.stride, syn.ReplayClip(scan),
                          syn.ReplaySeg(scan), index_offset=box[0], defer_frames=False).cuda()
    for f in scan.frames:
        full.integrate_features(f["depth"].cuda(), f["rgb"].cuda(), f["pose"].cuda(), f["K"].cuda(), f["feat"].cuda(),
                                [f["labels"].float().cuda()])
    for name in NAMES:
        side = "tsdf_weight" if name in ("tsdf", "tsdf_weight") else "weight"
        w1, w2 = _crop(before_1[side], box_1, box) > 0, _crop(before_2[side], box_2, box) > 0
        both, only_1, only_2 = w1 & w2, w1 & ~w2, ~w1 & w2
        if name == "weight":  # a condition of the test: all three kinds of voxel
            assert int(both.sum()) > 500 and int(only_1.sum()) > 50 and int(only_2.sum()) > 100, (int(both.sum()), int(only_1.sum()), int(only_2.sum()))
        got, want = getattr(fz, name), getattr(full, name)
        if name in ("weight", "tsdf_weight", "labels_one_hot"):
            assert torch.equal(got[both], want[both]), f"{name}: counts where both scans saw the voxel"
        elif name == "clip_feat":
            _feat_close(got[both], want[both], 1e-4, "clip_feat where both scans saw the voxel")
        else:
            assert float((got[both] - want[both]).abs().max()) <= 1e-4, f"{name} where both scans saw the voxel"
        assert torch.equal(_bits(got)[only_1], _bits(_crop(before_1[name], box_1, box))[only_1]), f"{name}: only the first scan's"
        assert torch.equal(_bits(got)[only_2], _bits(_crop(before_2[name], box_2, box))[only_2]), f"{name}: only the second scan's"

    # ---- the stages behind the fusion, run again on that volume
    grid = fz.label_index().view(*box[1])
    assert torch.equal(res.onehot_to_index, grid) and int((grid >= 0).sum()) > 1000
    knowledge, obj = discover_objects(grid, names, colors, arrays=True)
    assert torch.equal(res.voxel_obj_idx, obj) and torch.equal(fz.voxel_obj_idx, obj)
    assert list(res.scene_knowledge["unique_objects"]) == list(knowledge["unique_objects"]) and len(knowledge["unique_objects"]) >= 3
    verts, faces = fz.extract_mesh()[:2]
    assert np.array_equal(res.verts, verts) and np.array_equal(res.faces, faces) and len(faces) > 1000
    assert res.verts[:, 0].max() > 1.5, "nothing of the room the second session saw is in the mesh"


@pytest.mark.parametrize("lo,hi,unseen_at_least", [pytest.param(N_OLD, N_ALL, 0, id="the-second-half"),
                                                    pytest.param(N_ALL - 1, N_ALL, 1, id="its-last-frame-alone")])
def test_join_scenes_keeps_identities(rows_form, lo, hi, unseen_at_least):
    """``keep_identities=True``: the joined volume's objects are matched against the first reconstruction's, and an object of the
    first that the second never saw -- no voxel of it touched -- is reported unchanged.  The whole second half sees something of every
    object of the first scan (the condition is printed; the claim is empty there), so the join is also run with a second session of
    one frame, which leaves whole objects unseen: a condition of that case."""
    from spatially_aware_ai_amd.scene import join_scenes, reconstruct_scene
    from test_object_match_gpu import KNOBS

    scan = _scan()
    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    clip, seg = syn.ReplayClip(scan, class_names=names), syn.ReplaySeg(scan)
    config = {"voxel_size": 0.08, "trunc_vox": 3, "clip_patch_size": scan.patch, "clip_patch_stride": scan.stride}
    first = reconstruct_scene(_Part(scan, 0, N_OLD), config, clip, seg, names, colors)
    clip.calls = seg.calls = lo  # (the replay backbones answer frame after frame)
    second = reconstruct_scene(_Part(scan, lo, hi), config, clip, seg, names, colors, lattice_of=first)
    box_1, box_2 = _box(first.fusion), _box(second.fusion)
    grid_1 = first.voxel_obj_idx.clone().reshape(-1)
    seen_2 = _crop(second.fusion.weight, box_2, box_1) > 0  # over the first scan's box: voxels the second scan touched
    uo_prev = first.scene_knowledge["unique_objects"]
    unseen = [key for key, info in uo_prev.items()
              if bool((grid_1 == info["object_index"]).any()) and not bool(((grid_1 == info["object_index"]) & seen_2).any())]
    res = join_scenes(first, second, names, colors, keep_identities=True, identity_knobs=KNOBS)
    m = res.object_matches
    assert m is not None and res.seconds["identities"] > 0 and res.seconds["absorb"] > 0 and res.scene_knowledge["scan_version"] == 1
    assert res.fusion is first.fusion and clip.calls == hi, "a frame went through the backbones again"
    know = res.scene_knowledge
    for k in ("unchanged_objects", "moved_objects", "new_objects", "missing_objects"):
        assert k in know, k
    assert set(know["unchanged_objects"]) <= set(uo_prev) and not set(know["new_objects"]) & set(uo_prev)
    print("objects of the first scan:", len(uo_prev), "never seen by the second:", unseen,
          {k: len(getattr(m, k)) for k in ("kept", "absorbed", "moved", "new", "missing")})
    assert len(unseen) >= unseen_at_least and len(unseen) < len(uo_prev), "the case does not have both kinds of object"
    for key in unseen:
        assert key in know["unchanged_objects"], f"{key}: untouched by the second scan, and not reported unchanged"
        assert key in know["unique_objects"]
