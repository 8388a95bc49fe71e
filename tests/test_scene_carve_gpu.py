"""GPU: ``extend_scene(carve=True)`` -- an object that left the room, or stands elsewhere, in a later scan version is taken out of
the volume on the evidence of the new frames' depth (``fusion.observe_free_space`` / ``fusion.carve``), so that the
identity report (``keep_identities``) no longer finds it where it stood -- the one that left is missing; the one that moved is, under
``assign_identities``'s default knobs, missing + new --; with ``carve=False`` the ghost stays and is filed as unchanged,
which is what these tests measure the feature against.  f32, 64 x 48, D = 64, 32 + 16 frames, 8 cm voxels."""
import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import synthetic as syn

import carve_reference as ref

pytestmark = pytest.mark.gpu

W, H, DIM, N_OLD, N_NEW = 64, 48, 64, 32, 16
VOXEL, TRUNC_VOX = 0.08, 3
CHAIR = syn.SCENE_SURFACE_CLASSES[0]
# (every sphere's truncation shell stays clear of the walls' -- |coordinate| < 1.2 - 2 x 0.24 --, and the shells of the moved pair
#  are disjoint: centres 1.07 m apart, 0.3 + 0.25 + 2 x 0.24 = 1.03)
GONE = ((0.1, 0.0, -0.1), 0.5)
MOVED_FROM, MOVED_TO = ((0.4, 0.3, 0.0), 0.3), ((-0.45, -0.35, 0.0), 0.25)


class _Joined:
    """Two scan versions behind one pair of replay backbones: the frames in the order the flow fuses them."""

    def __init__(self, *scans):
        self.emb = scans[0].emb
        self.frames = [f for s in scans for f in s.frames]


def _versions(sphere_0, sphere_1):
    v0 = syn.SyntheticScan(31, N_OLD, W, H, DIM, sphere=sphere_0)
    v1 = syn.SyntheticScan(32, N_NEW, W, H, DIM, sphere=sphere_1)
    return v0, v1


def chair_id(res):
    return [k for k, o in res.scene_knowledge["unique_objects"].items() if int(o["class_id"]) == CHAIR]


def _flow(v0, v1, carve):
    from spatially_aware_ai_amd.scene import extend_scene, reconstruct_scene

    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    both = _Joined(v0, v1)
    clip, seg = syn.ReplayClip(both, class_names=names), syn.ReplaySeg(both)
    config = {"voxel_size": VOXEL, "trunc_vox": TRUNC_VOX, "clip_patch_size": v0.patch, "clip_patch_stride": v0.stride}
    first = reconstruct_scene(v0, config, clip, seg, names, colors)
    chairs = chair_id(first)
    assert len(chairs) == 1, f"version 0 does not hold exactly one chair: {chairs}"
    res = extend_scene(first, v1, config, clip, seg, names, colors, keep_identities=True, carve=carve)
    assert clip.calls == N_OLD + N_NEW and seg.calls == N_OLD + N_NEW, "a frame went through the backbones more than once"
    k = res.scene_knowledge
    print(f"carve={carve}: chair of version 0 {chair_id(first)}; " + "; ".join(f"{n} {list(k[n])}" for n in ("unchanged_objects", "moved_objects",
          "new_objects", "missing_objects")) + f"; carved {None if res.carve is None else int(res.carve.n_carved)}")
    assert res.scene_knowledge["scan_version"] == 1
    return first, res, chairs[0]


def _chairs(res):
    return {k: o for k, o in res.scene_knowledge["unique_objects"].items() if int(o["class_id"]) == CHAIR}


def _centres(fz):
    ax = [fz._buffers[f"axis_{a}"].cpu().double() for a in "xyz"]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3)


def _shell(fz, sphere):
    """Boolean [N] (CPU): the voxels within the truncation distance of ``sphere``'s surface."""
    centre, radius = sphere
    d = (_centres(fz) - torch.tensor(centre, dtype=torch.float64)).norm(dim=1)
    return ((d - radius).abs() <= TRUNC_VOX * VOXEL).numpy()


def _seen_through(oracle, fz, v1, min_views=2, max_support=0):
    """Boolean [N]: the voxels that at least ``min_views`` of the new frames look through and at most ``max_support`` support, by the
    oracle's classification of the eroded depth -- whatever the voxel holds."""
    grid = syn.GridSpec(torch.as_tensor(fz.origin).cpu().float(), VOXEL, fz.nvox.int(), TRUNC_VOX * VOXEL)
    vol = ref.oracle_volume(oracle, grid, axes=[fz._buffers[f"axis_{a}"] for a in "xyz"])
    depth = torch.stack([f["depth"][0] for f in v1.frames]).numpy()
    poses = torch.stack([f["pose"][0] for f in v1.frames]).numpy()
    K = torch.stack([f["K"][0] for f in v1.frames]).numpy()
    seen, hit = ref.evidence(vol, ref.erode(depth, 1), poses, K, np.ones(int(fz.nvox.prod()), dtype=np.int32))
    return (seen >= min_views) & (hit <= max_support)


def test_an_object_that_left_the_room_is_carved_and_filed_as_missing(oracle, rows_form):
    v0, v1 = _versions(GONE, None)
    first, res, chair = _flow(v0, v1, carve=True)
    fz = res.fusion
    assert res.carve is not None and res.seconds["carve"] > 0 and int(res.carve.n_carved) >= 200
    assert res.carve.evidence.n_frames == N_NEW and (res.carve.min_views, res.carve.max_support) == (2, 0)
    ghost = _shell(fz, GONE) & _seen_through(oracle, fz, v1)
    assert ghost.sum() >= 200, "the new frames see through too little of the sphere's shell: the test means nothing"
    weight = fz.weight.cpu().numpy()
    assert not (weight[ghost] > 0).any(), f"{int((weight[ghost] > 0).sum())} voxels of the sphere's shell that the new frames see through are still fused"
    assert chair in res.scene_knowledge["missing_objects"], (chair, list(res.scene_knowledge["missing_objects"]))
    assert chair not in res.scene_knowledge["unique_objects"] and not _chairs(res), "a chair was discovered again"
    assert chair in res.object_matches.missing
    # the same flow without the carve: the ghost stays where it stood and is filed as unchanged
    _, plain, chair_ = _flow(v0, v1, carve=False)
    assert chair_ == chair and plain.carve is None and "carve" not in plain.seconds
    assert chair in plain.scene_knowledge["unchanged_objects"] and chair not in plain.scene_knowledge["missing_objects"]
    w_plain = plain.fusion.weight.cpu().numpy()
    assert (w_plain[_shell(plain.fusion, GONE) & _seen_through(oracle, plain.fusion, v1)] > 0).sum() >= 200, "no ghost without the carve"


def test_an_object_that_stands_elsewhere_leaves_nothing_at_its_old_place(oracle, rows_form):
    """The filing under ``assign_identities``'s default knobs is asserted as it comes out: missing + new (see below)."""
    v0, v1 = _versions(MOVED_FROM, MOVED_TO)
    first, res, chair = _flow(v0, v1, carve=True)
    fz = res.fusion
    old_place = _shell(fz, MOVED_FROM)
    ghost = old_place & _seen_through(oracle, fz, v1)
    assert ghost.sum() >= 100
    assert not (fz.weight.cpu().numpy()[ghost] > 0).any()
    # no object remains at the old place: no voxel of the old shell belongs to a chair, and every chair lies at the new one
    obj = torch.as_tensor(res.voxel_obj_idx).reshape(-1).cpu().numpy()
    chairs = _chairs(res)
    assert len(chairs) == 1, list(chairs)
    chair_index = [int(o["object_index"]) for o in chairs.values()]
    assert not np.isin(obj[old_place], chair_index).any(), "a chair's voxels lie in the old sphere's shell"
    assert np.isin(obj[_shell(fz, MOVED_TO)], chair_index).sum() >= 50
    xyz = _centres(fz)[np.isin(obj, chair_index)]
    to_old = (xyz - torch.tensor(MOVED_FROM[0], dtype=torch.float64)).norm(dim=1)
    to_new = (xyz - torch.tensor(MOVED_TO[0], dtype=torch.float64)).norm(dim=1)
    assert bool((to_new < to_old).all()) and float(to_new.max()) < 0.6, "a chair's voxel lies away from the new sphere"
    # the identity.  The flow's expected filing is moved_objects; under assign_identities's DEFAULT knobs it comes out as missing +
    # new.  Both objects are of the chair's class and the member counts pass size_ratio_min = 0.5 (638 of 1058 on an MI355X, printed
    # below), so of rule 3 it is the descriptors' cosine that stays below cos_min = 0.9: a sphere of 0.3 m covers a cell or two of
    # the 5 x 7 feature map, whose cells mix in the walls behind it.  The rule and its knobs are not this test's to change: what
    # they give is asserted.
    k = res.scene_knowledge
    (new_chair, entry), = chairs.items()
    n_old, n_new = len(first.scene_knowledge["unique_objects"][chair]["voxels"]), len(entry["voxels"])
    print(f"chair members: version 0 {n_old}, version 1 {n_new}, ratio {n_new / n_old:.3f}")
    assert chair in k["missing_objects"] and new_chair in k["new_objects"] and new_chair != chair and not k["moved_objects"], \
        {n: list(k[n]) for n in ("unchanged_objects", "moved_objects", "new_objects", "missing_objects")}
    assert n_new >= 0.5 * n_old, "the member counts would explain the filing: the comment above is out of date"
    # without the carve the old chair stays where it stood and is filed as unchanged
    _, plain, _ = _flow(v0, v1, carve=False)
    kp = plain.scene_knowledge
    assert chair in kp["unchanged_objects"] and chair not in kp["missing_objects"] and not kp["moved_objects"]
    ghost_index = [int(o["object_index"]) for o in _chairs(plain).values()]
    obj_p = torch.as_tensor(plain.voxel_obj_idx).reshape(-1).cpu().numpy()
    assert np.isin(obj_p[_shell(plain.fusion, MOVED_FROM)], ghost_index).sum() >= 200, "no ghost at the old place without the carve"
