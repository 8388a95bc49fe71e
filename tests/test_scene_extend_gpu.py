"""GPU: a later scan version fused into the volume the first one left (``scene.extend_scene``): the box grows on the module's own
lattice (``lattice_box``, ``move_grid``), only the new frames go through the backbones, and what comes out is the volume -- and
the labels, objects and mesh -- of a module that held the larger box from the start."""
import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import synthetic as syn

pytestmark = pytest.mark.gpu

W, H, DIM, N_OLD, N_ALL = 64, 48, 64, 32, 48
NAMES = ("tsdf", "tsdf_weight", "weight", "rgb", "clip_feat", "labels_one_hot")


class _Part(torch.utils.data.Dataset):
    """Frames [first, last) of a scan, in the shape of the reference's loaders."""

    def __init__(self, scan, first, last):
        self.scan, self.first, self.n = scan, first, last - first
        self.imwidth, self.imheight = scan.imwidth, scan.imheight

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.scan[self.first + i]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def test_extend_scene_fuses_only_the_new_frames_into_the_grown_box(rows_form):
    from spatially_aware_ai_amd.clip_seem_fusion import ClipSeemFusion, discover_objects
    from spatially_aware_ai_amd.scene import extend_scene, reconstruct_scene

    scan = syn.SyntheticScan(23, N_ALL, W, H, DIM)
    for f in scan.frames[N_OLD:]:  # the headset walks on: the later frames see the room half a metre further along x and y
        f["pose"] = f["pose"].clone()
        f["pose"][0, :3, 3] += torch.tensor([0.5, -0.4, 0.0])
    names, colors = syn.scene_class_names(), syn.scene_class_colors()
    clip, seg = syn.ReplayClip(scan, class_names=names), syn.ReplaySeg(scan)
    config = {"voxel_size": 0.08, "trunc_vox": 3, "clip_patch_size": scan.patch, "clip_patch_stride": scan.stride}
    first = reconstruct_scene(_Part(scan, 0, N_OLD), config, clip, seg, names, colors)
    assert clip.calls == N_OLD and seg.calls == N_OLD and first.scene_knowledge["scan_version"] == 0
    fz = first.fusion
    old_box = (fz.index_offset, tuple(int(v) for v in fz.nvox))
    res = extend_scene(first, _Part(scan, N_OLD, N_ALL), config, clip, seg, names, colors)
    assert clip.calls == N_ALL and seg.calls == N_ALL, "the backbones saw more than the new frames"
    assert res.fusion is fz and res.scene_knowledge["scan_version"] == 1
    for k in ("bounds", "move_grid", "fuse", "label_argmax", "objects", "extract_mesh", "object_meshes"):
        assert res.seconds[k] > 0, k
    new_box = (fz.index_offset, tuple(int(v) for v in fz.nvox))
    assert torch.equal(torch.as_tensor(res.nvox), fz.nvox) and all(v % 4 == 0 for v in new_box[1])
    lo_in = [o - n for o, n in zip(old_box[0], new_box[0])]  # the old box's low corner in the new box's indices
    assert all(v >= 0 for v in lo_in) and all(l + a <= b for l, a, b in zip(lo_in, old_box[1], new_box[1])), "the old box is not inside"
    assert new_box[1][0] >= old_box[1][0] + 4 and new_box[0][1] <= -3, "the scan did not grow: the test means nothing"
    assert tuple(res.xyz.shape)[0] > tuple(first.xyz.shape)[0]

    # ---- the volume: fresh modules over the new box, fed frame after frame
    def fresh(frames):
        m = ClipSeemFusion(first.origin, 0.08, torch.tensor(new_box[1]), 3 * 0.08, False, scan.patch, scan.stride,
                           syn.ReplayClip(scan), syn.ReplaySeg(scan), index_offset=new_box[0], defer_frames=False).cuda()
        for f in frames:
            m.integrate_features(f["depth"].cuda(), f["rgb"].cuda(), f["pose"].cuda(), f["K"].cuda(), f["feat"].cuda(),
                                 [f["labels"].float().cuda()])
        return m

    full, late = fresh(scan.frames), fresh(scan.frames[N_OLD:])
    inside = torch.zeros(new_box[1], dtype=torch.bool, device="cuda")
    inside[tuple(slice(l, l + a) for l, a in zip(lo_in, old_box[1]))] = True
    inside = inside.reshape(-1)
    assert int(((late.weight > 0) & ~inside).sum()) > 500 and int(((fz.weight > 0) & inside).sum()) > 500
    for name in NAMES:
        got, f, l = getattr(fz, name), getattr(full, name), getattr(late, name)
        assert torch.equal(_bits(got)[inside], _bits(f)[inside]), f"{name}: inside the old box, against all 48 frames fused over the new one"
        assert torch.equal(_bits(got)[~inside], _bits(l)[~inside]), f"{name}: outside the old box, against the new frames alone"

    # ---- the stages behind the fusion, run again on that volume
    grid = fz.label_index().view(*new_box[1])
    assert torch.equal(res.onehot_to_index, grid) and int((grid >= 0).sum()) > 1000
    knowledge, obj = discover_objects(grid, names, colors, arrays=True)
    assert torch.equal(res.voxel_obj_idx, obj) and torch.equal(fz.voxel_obj_idx, obj)
    assert list(res.scene_knowledge["unique_objects"]) == list(knowledge["unique_objects"]) and len(knowledge["unique_objects"]) >= 3
    verts, faces = fz.extract_mesh()[:2]
    assert np.array_equal(res.verts, verts) and np.array_equal(res.faces, faces) and len(faces) > 1000
    # the mesh lies where the box is: vertex = (index in the box + the box's offset) * voxel + origin
    vi, _ = fz._marching_cubes_vertices()
    want = (vi + np.asarray(new_box[0], dtype=vi.dtype)) * 0.08 + torch.as_tensor(fz.origin).cpu().numpy()
    assert np.array_equal(res.verts, want)
    lo = np.array([float(fz.axis_x[0]), float(fz.axis_y[0]), float(fz.axis_z[0])])
    hi = np.array([float(fz.axis_x[-1]), float(fz.axis_y[-1]), float(fz.axis_z[-1])])
    assert (res.verts >= lo - 1e-4).all() and (res.verts <= hi + 1e-4).all()
    assert res.verts[:, 0].max() > 1.5, "nothing of the room the later frames saw is in the mesh"
