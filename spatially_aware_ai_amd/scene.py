"""The scene-level flow of the reference's manager on the MI355X path, stage by stage and timed.

``reconstruct_scene`` is ``InSituManager.run_clipfusion`` (reference clip_seem_fusion.py:247-437) in the reference's own
order -- bounds from a sparse back-projection, one ``integrate`` call per frame, label decode, object discovery, the
attributes the manager sets on the volume from outside, ``extract_mesh``'s 6-tuple, per-object meshes, artefacts on disk --
and ``SceneResult.text_query`` is ``InSituManager.clip_text_query`` (:482-561) over what the reconstruction left.  Every
stage is one of the package's existing entry points (nothing is computed here that the hot path does not already own);
what this module adds is the chain and a wall-clock split per stage, the counterpart of the reference's one published
performance statement ("within a few minutes after a user scans the environment", README.md:4).  ``extend_scene`` fuses a later
scan version's new frames into the volume a reconstruction left (not in the reference, which fuses every version from its
first frame); ``join_scenes`` puts two reconstructions of one lattice together (``reconstruct_scene(lattice_of=...)``,
``fusion.absorb``); ``coarsen_scene`` takes a reconstruction to a whole multiple of its voxel size (``fusion.coarsen``), ``resample_scene`` to any other
lattice under a rigid transform (``fusion.resample``).

The Flask app, the datasets' decoders and the DGCNN in-situ learner stay the reference's.
"""
from __future__ import annotations

import json
import os
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from .clip_seem_fusion import ClipSeemFusion, TextQueryEngine, discover_objects, extract_mesh_by_object
from ._lib import SafError
from .clipfusion import backproject_pcd, lattice_box, scene_bounds
from .io import ArrayList, dumps_scene_knowledge, save_npy, save_ply, save_scene_arrays


@dataclass
class SceneResult:
    """What ``run_clipfusion`` leaves on the manager (clip_seem_fusion.py:322-424), plus the stage clock."""

    fusion: ClipSeemFusion
    origin: torch.Tensor
    nvox: torch.Tensor
    xyz: torch.Tensor  # the sparse preview cloud (clip_seem_fusion.py:269-275)
    onehot_to_index: torch.Tensor  # [nx,ny,nz] int64 on the device
    scene_knowledge: dict
    voxel_obj_idx: torch.Tensor
    verts: np.ndarray
    faces: np.ndarray
    vertex_colors: torch.Tensor
    vert_clip_feat: torch.Tensor
    vertex_obj_idx: torch.Tensor
    segmentation_color: torch.Tensor
    paths: dict = field(default_factory=dict)
    seconds: dict = field(default_factory=dict)
    engine: TextQueryEngine | None = None
    objects: object | None = None  # objects.ObjectDescriptors, computed by the first object_query
    object_matches: object | None = None  # objects.ObjectMatches of extend_scene(keep_identities=True)
    carve: object | None = None  # clipfusion.CarveResult of extend_scene(carve=True)

    def text_query(self, clip_model, text):
        """``clip_text_query`` (clip_seem_fusion.py:482-561): RGBA heat map over the scene mesh, or None."""
        t0 = time.perf_counter()
        if self.engine is None:
            self.engine = TextQueryEngine(clip_model, self.vert_clip_feat, verts=self.verts.tolist(), faces=self.faces.tolist(),
                                          scene_knowledge=self.scene_knowledge)
        out = self.engine.clip_text_query(text)
        torch.cuda.synchronize()
        self.seconds["text_query"] = self.seconds.get("text_query", 0.0) + time.perf_counter() - t0
        return out

    def render_query(self, clip_model, text, pose, K, height, width):
        """The text query seen from a camera (what the reference's AR client overlays on its view, app_unity.py): an RGBA image
        [H,W,4] (numpy f32) -- ``text`` against the scene's object classes as in ``text_query``, softmax relevance of ``text``
        (the last column) per pixel through ``relevance_to_rgba``; alpha 0 where the pixel sees nothing of the volume."""
        from .clip_seem_fusion import relevance_to_rgba

        t0 = time.perf_counter()
        uo = self.scene_knowledge.get("unique_objects", {})
        names = sorted(set(uo[k]["class_label"] for k in uo) - {text}) + [text]
        feats = clip_model.encode_text_with_prompt_ensemble(names, "cpu", prompt_templates=["a photo of {}"])
        out = self.fusion.render_query(feats, pose, K, height, width, epilogue="softmax", rgb=False)
        rel = out.relevance[..., -1].reshape(-1).cpu().numpy()
        rgba = relevance_to_rgba(rel).astype(np.float32).reshape(int(height), int(width), 4)
        rgba[~out.hit.cpu().numpy()] = 0.0
        self.seconds["render_query"] = self.seconds.get("render_query", 0.0) + time.perf_counter() - t0
        return rgba

    def object_query(self, clip_model, text):
        """The text query answered per OBJECT (objects.ObjectQueryResult): ``text`` against the scene's object classes, labels
        chosen exactly as ``render_query`` chooses them; ``best(n)`` names the most relevant objects with their centroid and
        box.  The descriptors (one reduction over the volume, ``objects.describe_objects``) are computed by the first call.
        They are kept in ``self.objects`` and NOT recomputed when the scene knowledge changes: after ``merge_objects(...,
        voxel_obj_idx=...)`` or a change of an object's ``removed`` flag assign ``self.objects = self.objects.merged(...)`` or
        set ``self.objects = None`` (the next call describes the objects again)."""
        from .objects import describe_objects

        t0 = time.perf_counter()
        if self.objects is None:
            self.objects = describe_objects(self.fusion, self.voxel_obj_idx, self.scene_knowledge)
        uo = self.scene_knowledge.get("unique_objects", {})
        names = sorted(set(uo[k]["class_label"] for k in uo) - {text}) + [text]
        feats = clip_model.encode_text_with_prompt_ensemble(names, "cpu", prompt_templates=["a photo of {}"])
        out = self.objects.query(feats, epilogue="softmax")
        torch.cuda.synchronize()
        self.seconds["object_query"] = self.seconds.get("object_query", 0.0) + time.perf_counter() - t0
        return out


class FrameStager:
    """Host -> device staging of the loader's frames through a few reusable pinned buffers.

    The reference's loop calls ``.to(device)`` on the four freshly collated tensors of every frame
    (clip_seem_fusion.py:305-311).  On ROCm a copy from pageable memory pins the source pages for the transfer, and the
    DataLoader frees the batch right after: measured 6.6 ms per 640 x 480 frame for the four copies (tools/probe_scene.py),
    against 0.07 ms for the fused path to consume the frame.  Here the batch is copied into one of ``slots`` pinned buffers
    (a host memcpy) and sent from there asynchronously on the current stream; a slot is reused once its last transfer has
    completed (an event per slot).  What ``integrate`` receives is the same tensors on the device."""

    def __init__(self, device, slots=4):
        self.device = torch.device(device)
        self.slots = int(slots)
        self._bufs = {}
        self._events = [None] * self.slots
        self._k = 0

    def __call__(self, *tensors):
        k = self._k
        self._k = (k + 1) % self.slots
        if self._events[k] is not None:
            self._events[k].synchronize()
        out = []
        for i, t in enumerate(tensors):
            key = (k, i, tuple(t.shape), t.dtype)
            buf = self._bufs.get(key)
            if buf is None:
                self._bufs = {kk: v for kk, v in self._bufs.items() if kk[:2] != (k, i)}  # another shape took this place
                buf = self._bufs[key] = torch.empty(t.shape, dtype=t.dtype).pin_memory()
            buf.copy_(t)
            out.append(buf.to(self.device, non_blocking=True))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._events[k] = ev
        return out


class _Clock:
    def __init__(self):
        self.seconds = {}
        self._t = None

    def start(self):
        torch.cuda.synchronize()
        self._t = time.perf_counter()

    def lap(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.seconds[name] = self.seconds.get(name, 0.0) + now - self._t
        self._t = now


def _fuse_one_by_one(fusion, dataset, config, device, num_workers):
    """The fusion loop, one frame per ``integrate`` call (clip_seem_fusion.py:303-313); returns where the host's time went."""
    loader = torch.utils.data.DataLoader(dataset, batch_size=1, num_workers=num_workers)
    stage = FrameStager(device)
    refine_poses = bool(config.get("refine_poses", False))  # not in the reference's config: poses that drift (headsets)
    host = {"loader": 0.0, "stage": 0.0, "integrate": 0.0}  # where the host's time in the loop goes (no device sync inside)
    t_prev = time.perf_counter()
    for rgb_imgs, depth_imgs, poses, K, _ in loader:
        t0 = time.perf_counter()
        depth_d, rgb_d, poses_d, k_d = stage(depth_imgs.float(), rgb_imgs.float(), poses.float(), K.float())
        t1 = time.perf_counter()
        if refine_poses:  # (each frame is refined against the volume so far: no deferred queue)
            fusion.integrate_refined(depth_d, rgb_d, poses_d, k_d)
        else:
            fusion.integrate(depth_d, rgb_d, poses_d, k_d)
        t2 = time.perf_counter()
        host["loader"] += t0 - t_prev
        host["stage"] += t1 - t0
        host["integrate"] += t2 - t1
        t_prev = t2
    return host


def _carve_by_frames(fusion, dataset, device, num_workers, knobs, batch_size=16):
    """Every frame of ``dataset`` observed against the volume as it stands (depth, pose and K: the backbones see nothing), then the
    carve applied once.  ``knobs``: ``min_views``, ``max_support``, ``erode`` of ``fusion.carve``."""
    knobs = dict(knobs or {})
    unknown = set(knobs) - {"min_views", "max_support", "erode"}
    if unknown:
        raise SafError(f"carve_knobs: unknown entries {sorted(unknown)} (min_views, max_support, erode)")
    erode = knobs.pop("erode", 1)
    evidence = None
    for _, depth_imgs, poses, K, _ in torch.utils.data.DataLoader(dataset, batch_size=batch_size, num_workers=num_workers):
        evidence = fusion.observe_free_space(depth_imgs.float().to(device), poses.float().to(device), K.float().to(device), erode=erode,
                                             evidence=evidence)
    if evidence is None:
        raise SafError("extend_scene(carve=True): the dataset holds no frame")
    return fusion.carve(evidence=evidence, **knobs)


def _after_fusion(fusion, origin, nvox, xyz, clk, class_names, class_colors, scan_version, out_dir, object_meshes,
                  marching_cubes, python_lists, prev=None, extra=None):
    """The stages behind the fusion loop (clip_seem_fusion.py:315-424, :563-607): labels, objects, the scene mesh, per-object
    meshes, artefacts -- shared by ``reconstruct_scene``, ``extend_scene``, ``join_scenes``, ``coarsen_scene`` and ``resample_scene`` (``extra``: entries
    it adds to ``scene_knowledge``).  ``clk`` has just lapped the fusion.  ``prev``
    (``_describe_version`` of the previous version, or None): the discovered objects take the previous version's identities
    before anything is built from their indices."""
    # ---- the volume's artefacts (save_files_and_broadcast, :566-581) start now, on a thread of their own: nothing below writes
    #      clip_feat or rgb (the lap above synchronised the device; ctypes releases the interpreter lock for the whole write)
    writer = None
    if out_dir is not None:
        import threading

        os.makedirs(out_dir, exist_ok=True)
        nx_, ny_, nz_ = (int(v) for v in fusion.nvox)
        vol_rgb, vol_feat = fusion.rgb.view(nx_, ny_, nz_, 3), fusion.clip_feat.view(nx_, ny_, nz_, -1)
        wpaths, werr = {}, []

        def _write_volume():
            try:
                t_w = time.perf_counter()
                with torch.cuda.device(vol_feat.device), torch.cuda.stream(torch.cuda.Stream(vol_feat.device)):
                    wpaths["voxel_rgb"] = save_npy(os.path.join(out_dir, "voxel_rgb.npy"), vol_rgb)
                    wpaths["voxel_clip_feats"] = save_npy(os.path.join(out_dir, "voxel_clip_feats.npy"), vol_feat)
                wpaths["_seconds"] = time.perf_counter() - t_w
            except BaseException as e:  # noqa: BLE001 -- re-raised by the main thread at the join
                werr.append(e)

        writer = threading.Thread(target=_write_volume, name="saf-scene-writer")
        writer.start()
    # ---- labels: argmax with the empty check (:315-333), on the device
    onehot_to_index = fusion.label_index().view(*[int(v) for v in fusion.nvox])
    clk.lap("label_argmax")
    # ---- objects (flood_fill_3d, :341-348) and the attributes the manager sets from outside (:351-372)
    scene_knowledge, voxel_obj_idx = discover_objects(onehot_to_index, class_names, class_colors, arrays=not python_lists)
    scene_knowledge["scan_version"] = scan_version
    scene_knowledge.update(extra or {})  # (what the caller knows about this version: coarsen_scene's grid)
    matches = None
    if prev is not None:
        clk.lap("objects")
        scene_knowledge, voxel_obj_idx, matches = _carry_version(fusion, prev, scene_knowledge, voxel_obj_idx)
        clk.lap("identities")
    fusion.unique_objects = scene_knowledge["unique_objects"]
    fusion.voxel_obj_idx = voxel_obj_idx
    seg_color = torch.clone(fusion.rgb).view(*[int(v) for v in fusion.nvox], -1)
    for obj_info in scene_knowledge["unique_objects"].values():
        if obj_info["color"] is None:
            continue
        vox = torch.as_tensor(np.asarray(obj_info["voxels"], dtype=np.int64), device=seg_color.device)
        color = torch.tensor(obj_info["color"]).float() / 255.0
        seg_color[vox[:, 0], vox[:, 1], vox[:, 2]] = color.to(seg_color.device)
    fusion.objects_segmentation_color = seg_color.view(-1, 3)
    clk.lap("objects")
    # ---- the scene mesh with per-vertex colour, feature, object index, segment colour (:377-385)
    verts, faces, vertex_colors, vertex_clip_feats, vertex_obj_idx, segmentation_color = fusion.extract_mesh(marching_cubes)
    clk.lap("extract_mesh")
    # ---- per-object meshes into the scene knowledge (:393-417)
    if object_meshes:
        vc_h, vo_h = vertex_colors.cpu().numpy(), vertex_obj_idx.cpu().numpy()
        for obj_key, obj_value in scene_knowledge["unique_objects"].items():
            ov, of_, oc, _ = extract_mesh_by_object(verts, faces, vc_h, vo_h, obj_value["object_index"])
            if python_lists:
                mesh = {"vertices": ov.tolist(), "faces": of_.tolist(), "colors": oc.tolist()}
            else:
                mesh = {"vertices": ArrayList(ov), "faces": ArrayList(of_), "colors": ArrayList(oc)}
            scene_knowledge["unique_objects"][obj_key]["mesh"] = None if len(of_) < 10 else mesh
        clk.lap("object_meshes")
    res = SceneResult(fusion, origin, nvox, xyz, onehot_to_index, scene_knowledge, voxel_obj_idx, verts, faces, vertex_colors,
                      vertex_clip_feats, vertex_obj_idx, segmentation_color, object_matches=matches)
    # ---- artefacts (save_files_and_broadcast, :563-607)
    if out_dir is not None:
        res.paths = {"vertex_clip_feats": save_npy(os.path.join(out_dir, "vertex_clip_feats.npy"), torch.as_tensor(vertex_clip_feats)),
                     "vertex_obj_idx": save_npy(os.path.join(out_dir, "vertex_obj_idx.npy"), torch.as_tensor(vertex_obj_idx))}
        res.paths["mesh_rgb"] = save_ply(os.path.join(out_dir, "mesh_rgb.ply"), verts, faces, vertex_colors)
        res.paths["mesh_segmentation"] = save_ply(os.path.join(out_dir, "mesh_segmentation.ply"), verts, faces, segmentation_color)
        res.paths["scene_knowledge"] = os.path.join(out_dir, "scene_knowledge.json")
        with open(res.paths["scene_knowledge"], "w") as f:
            # the same text as json.dump(scene_knowledge, f, default=str) (clip_seem_fusion.py:603-604) -- but json.dump
            # walks the object with the pure-Python encoder, a chunk at a time: 2.1 s for this scene's voxel lists and
            # meshes; dumps() hands the whole object to the C encoder: 0.5 s
            # and the bulky lists (voxels, per-object meshes) are arrays rendered natively: 0.05 s
            f.write(dumps_scene_knowledge(scene_knowledge))
        clk.lap("save")
        writer.join()
        if werr:
            raise werr[0]
        clk.seconds["volume_write_beside"] = round(wpaths.pop("_seconds"), 4)
        res.paths.update(wpaths)
        clk.lap("save_volume_wait")
    return res


def _describe_version(fusion, result, knobs):
    """What ``_carry_version`` needs of the version ``result`` describes, taken while ``fusion`` still holds that version's box:
    the objects' descriptors, their slot grid and the box."""
    from .objects import describe_objects, object_slots

    desc = describe_objects(fusion, result.voxel_obj_idx, result.scene_knowledge)
    dev = fusion._buffers["weight"].device
    slot, _ = object_slots(torch.as_tensor(result.voxel_obj_idx).to(dev), result.scene_knowledge)
    return {"desc": desc, "slot": slot.contiguous(), "index_offset": tuple(int(v) for v in fusion.index_offset),
            "nvox": tuple(int(v) for v in fusion.nvox), "knowledge": result.scene_knowledge, "knobs": dict(knobs or {})}


def _carry_version(fusion, prev, scene_knowledge, voxel_obj_idx):
    """The new labelling under the previous version's identities (objects.py): descriptors of the new objects, the
    overlap table of the two slot grids on their shared lattice, the match, the bookkeeping."""
    from .objects import carry_identities, describe_objects, match_objects, object_overlap, object_slots

    desc = describe_objects(fusion, voxel_obj_idx, scene_knowledge)
    overlap = None
    if len(prev["desc"]) and len(desc):
        slot, _ = object_slots(voxel_obj_idx, scene_knowledge)
        off = tuple(n - o for n, o in zip(fusion.index_offset, prev["index_offset"]))
        overlap = object_overlap(prev["slot"], prev["nvox"], slot.contiguous(), tuple(int(v) for v in fusion.nvox), off,
                                 len(prev["desc"]), len(desc))
    matches = match_objects(prev["desc"], desc, overlap, prev["knowledge"], scene_knowledge, **prev["knobs"])
    scene_knowledge, voxel_obj_idx = carry_identities(prev["knowledge"], scene_knowledge, voxel_obj_idx, matches)
    return scene_knowledge, voxel_obj_idx, matches


def _scene_box(xyz, voxel_size, trunc_m, lattice_of=None):
    """(origin, nvox, index_offset) of a new scene's volume: ``scene_bounds`` of its cloud, or -- ``lattice_of``, a ``SceneResult``
    -- the box of that result's lattice around the cloud alone (``lattice_box(..., union=False)``).  Host only."""
    if lattice_of is None:
        origin, nvox = scene_bounds(xyz, voxel_size, trunc_m)
        return origin, nvox, (0, 0, 0)
    base = lattice_of.fusion
    if float(base.voxel_size) != float(voxel_size) or float(base.trunc) != float(trunc_m):
        raise SafError(f"lattice_of: the scene was fused at voxel size {float(base.voxel_size)} and truncation {float(base.trunc)}, "
                       f"the config asks for {float(voxel_size)} and {float(trunc_m)}")
    index_offset, nvox = lattice_box(base, xyz, trunc_m=trunc_m, union=False)
    return base.origin, torch.tensor(nvox, dtype=torch.int32), index_offset


def reconstruct_scene(dataset, config, clip_model, seg_model, class_names, class_colors=None, device="cuda", out_dir=None,
                      max_depth=4, scale_patches_by_depth=False, feat_dtype=torch.float32, num_workers=0,
                      object_meshes=True, marching_cubes=None, python_lists=False, lattice_of=None):
    """``InSituManager.run_clipfusion`` (clip_seem_fusion.py:247-437).

    ``dataset`` yields the reference loaders' 5-tuple ``(rgb[H,W,3], depth[H,W], pose[4,4], K[3,3], idx)`` and has
    ``imwidth`` / ``imheight``; ``config`` needs ``voxel_size``, ``trunc_vox``, ``clip_patch_size``,
    ``clip_patch_stride`` (the reference's config dict, clip_seem_fusion.py:63-94).  ``class_names`` /
    ``class_colors`` are kMaX's ``COCO_PANOPTIC_CLASSES`` / ``COCO_PANOPTIC_COLORS`` in the reference
    (handy_utils.py:23-26).  Returns a ``SceneResult``; ``result.seconds`` holds the wall clock of every stage.

    ``python_lists``: keep the bulky members of ``scene_knowledge`` -- every object's ``voxels`` and ``mesh`` -- as the nested
    Python lists the reference builds (handy_utils.py:430-452, clip_seem_fusion.py:393-417); by default they are
    ``io.ArrayList``s around the arrays (same reads, same JSON: 0.8 s of a 2 s scan were spent building those lists and
    encoding them).  With ``out_dir`` the volume's ``.npy`` files (3.4 GB at the reference's largest grid) are written by a
    second thread from the moment the fusion is complete, beside the object / mesh stages.

    ``lattice_of`` (not in the reference; default None: the bounds above): a ``SceneResult`` on whose LATTICE the new volume is
    built -- its ``origin``, and the box ``lattice_box(lattice_of.fusion, xyz, union=False)`` of this scan's own cloud -- so that
    ``join_scenes`` can put the two together.  ``config`` must give the same voxel size and truncation distance."""
    clk = _Clock()
    clk.start()
    # ---- scene bounds (clip_seem_fusion.py:266-287)
    xyz, _ = backproject_pcd(dataset, batch_size=1, num_workers=num_workers, device="cpu", max_depth=max_depth)
    trunc_m = config["trunc_vox"] * config["voxel_size"]
    origin, nvox, index_offset = _scene_box(xyz, config["voxel_size"], trunc_m, lattice_of)
    clk.lap("bounds")
    # ---- the volume and the fusion loop, one frame per call (clip_seem_fusion.py:291-313)
    # (the reference builds the module on the host and moves it, clip_seem_fusion.py:291-302: gigabytes of zeros through pageable
    #  memory -- 0.7 s at the reference's largest grid; `device=` lets the buffers be born on the device)
    fusion = ClipSeemFusion(origin, config["voxel_size"], nvox, trunc_m, scale_patches_by_depth, config["clip_patch_size"],
                            config["clip_patch_stride"], clip_model, seg_model, feat_dtype=feat_dtype, index_offset=index_offset,
                            device=device).to(device)
    host = _fuse_one_by_one(fusion, dataset, config, device, num_workers)
    fusion.flush()
    clk.lap("fuse")
    clk.seconds["fuse_host_split"] = {k: round(v, 4) for k, v in host.items()}
    res = _after_fusion(fusion, origin, nvox, xyz, clk, class_names, class_colors, 0, out_dir, object_meshes, marching_cubes,
                        python_lists)
    res.seconds = clk.seconds
    return res


def extend_scene(result, dataset, config, clip_model, seg_model, class_names, class_colors=None, out_dir=None, max_depth=4,
                 num_workers=0, object_meshes=True, marching_cubes=None, python_lists=False, multiple=4, keep_identities=False,
                 identity_knobs=None, carve=False, carve_knobs=None):
    """A later version of a scan: fuse its NEW frames (``dataset`` holds only those) into ``result.fusion`` and run the stages
    behind the fusion again.  The reference's manager fuses every frame of every version into a new grid (``/reprocess_scan``,
    ``get_path(config, curr_ver, ...)``): the backbones, which cost far more than the fusion, see the whole scan again.  Here the
    new frames are back-projected, the volume is moved to the box of its own lattice that holds the old box and the new frames'
    bounds (``lattice_box(..., union=True)``, ``move_grid``: a copy), and only the new frames go through the backbones
    and the one-frame-per-call loop.  On the voxels of the old box the volume is bit for bit the one that would have fused all
    the frames into the new box from the start (in the frame-ordered form; the default form within its own rounding).

    ``clip_model`` / ``seg_model`` replace the module's backbones when they are other objects than the ones it holds; the other
    arguments are ``reconstruct_scene``'s.  Objects are discovered anew from the new labels; by default an object keeps no
    identity across versions.  Returns a new ``SceneResult`` around the same module -- ``result`` itself describes a box the module
    no longer holds --; ``scene_knowledge["scan_version"]`` counts on, ``seconds`` gains ``move_grid``.

    ``keep_identities``: the new version's objects are matched against ``result``'s (``objects.match_objects``: kept in place by
    voxel overlap, absorbed into a user's merge, moved by descriptor, new, missing; ``identity_knobs`` are
    ``objects.assign_identities``'s thresholds) and take their ids, indices, user labels and merges
    (``objects.carry_identities``) before the mesh and the per-object meshes are built: ``scene_knowledge`` gains
    ``unchanged_objects``, ``moved_objects``, ``new_objects`` and ``missing_objects`` without a trained in-situ model, the result
    ``object_matches``, ``seconds`` ``identities``.  The fused volume is the same either way.  A float16 module is refused
    (``describe_objects``).

    ``carve`` (default False: nothing changes): projective fusion only ever adds, so an object that was carried out of the room
    between the versions stays in the volume -- the new frames look through where it stood, which moves the TSDF there and leaves
    the weights, features and label histograms alone -- and is discovered again, in place, as "unchanged".  With ``carve=True``,
    after ``move_grid`` and before the new frames are fused, every new frame's depth is observed against the old voxels
    (``fusion.observe_free_space``) and what enough of them see through is taken out (``fusion.carve``): depth, pose
    and K only, no frame goes through a backbone for it.  ``carve_knobs``: ``min_views``, ``max_support`` and ``erode`` of
    ``fusion.carve``.  ``seconds`` gains ``carve``, the result ``carve`` (the ``CarveResult``)."""
    clk = _Clock()
    clk.start()
    fusion = result.fusion
    device = fusion._buffers["tsdf"].device
    if clip_model is not None and clip_model is not fusion.clip:
        fusion.clip = clip_model
    if seg_model is not None and seg_model is not fusion.segmentation_model:
        fusion.segmentation_model = seg_model
    xyz_new, _ = backproject_pcd(dataset, batch_size=1, num_workers=num_workers, device="cpu", max_depth=max_depth)
    index_offset, nvox = lattice_box(fusion, xyz_new, union=True, multiple=multiple)
    clk.lap("bounds")
    prev = None
    if keep_identities:  # the previous version's objects, described while the module still holds their box
        prev = _describe_version(fusion, result, identity_knobs)
        clk.lap("identities")
    fusion.move_grid(index_offset, nvox)
    clk.lap("move_grid")
    carved = None
    if carve:
        carved = _carve_by_frames(fusion, dataset, device, num_workers, carve_knobs)
        clk.lap("carve")
    host = _fuse_one_by_one(fusion, dataset, config, device, num_workers)
    fusion.flush()
    clk.lap("fuse")
    clk.seconds["fuse_host_split"] = {k: round(v, 4) for k, v in host.items()}
    version = int(result.scene_knowledge.get("scan_version", 0)) + 1
    res = _after_fusion(fusion, result.origin, fusion.nvox, torch.cat((result.xyz, xyz_new)), clk, class_names, class_colors, version,
                        out_dir, object_meshes, marching_cubes, python_lists, prev=prev)
    res.seconds = clk.seconds
    res.carve = carved
    return res


def join_scenes(result, other, class_names, class_colors=None, out_dir=None, object_meshes=True, marching_cubes=None,
                python_lists=False, multiple=4, keep_identities=False, identity_knobs=None):
    """Two reconstructions of ONE lattice put together (``other`` built with ``reconstruct_scene(..., lattice_of=result)``: two
    sessions in one room, a second headset, the far end of a corridor): ``result.fusion.absorb(other.fusion)`` -- the volume grows
    to the box around both and blends ``other``'s running means in by weights (saf_volume_absorb), no frame goes through
    the backbones again -- and the stages behind the fusion run again on the joined volume.  ``other`` and its module are unchanged.

    Returns a new ``SceneResult`` around ``result.fusion`` -- ``result`` itself describes a volume the module no longer holds --;
    ``xyz`` is the two clouds concatenated, ``scene_knowledge["scan_version"]`` counts on from ``result``'s, ``seconds`` gains
    ``absorb``.  ``multiple`` is ``absorb``'s; ``keep_identities`` / ``identity_knobs`` are ``extend_scene``'s: ``result``'s objects
    are described before the absorb and the joined volume's objects are matched against them."""
    clk = _Clock()
    clk.start()
    fusion = result.fusion
    prev = None
    if keep_identities:  # the previous version's objects, described while the module still holds their box
        prev = _describe_version(fusion, result, identity_knobs)
        clk.lap("identities")
    fusion.absorb(other.fusion, grow=True, multiple=multiple)
    clk.lap("absorb")
    version = int(result.scene_knowledge.get("scan_version", 0)) + 1
    res = _after_fusion(fusion, result.origin, fusion.nvox, torch.cat((result.xyz, other.xyz)), clk, class_names, class_colors, version,
                        out_dir, object_meshes, marching_cubes, python_lists, prev=prev)
    res.seconds = clk.seconds
    return res


def coarsen_scene(result, factor, class_names, class_colors=None, out_dir=None, object_meshes=True, marching_cubes=None,
                  python_lists=False):
    """A reconstruction at ``factor`` (2, 3 or 4) times its voxel size: ``result.fusion.coarsen(factor)`` -- every coarse voxel the
    weighted mean of the fine voxels it covers (saf_volume_coarsen), no frame goes through the backbones again -- and
    the stages behind the fusion run again on the coarse volume, which keeps fusing at the coarse size (``extend_scene``) and can
    be joined with a reconstruction fused at that size on the same coarse lattice (``join_scenes``).

    Returns a new ``SceneResult`` around ``result.fusion`` -- ``result`` itself describes a volume the module no longer holds --;
    ``origin`` and ``nvox`` are the coarse volume's, ``xyz`` is ``result``'s, ``scene_knowledge["scan_version"]`` counts on from
    ``result``'s, ``scene_knowledge`` gains ``voxel_size``, ``nvox`` and ``index_offset`` of the coarse volume (and so does
    ``scene_knowledge.json``), ``seconds`` gains ``coarsen``.  Objects are discovered anew from the coarse labels: an object keeps
    no identity across a coarsening (the overlap of objects across two lattices is not defined here)."""
    clk = _Clock()
    clk.start()
    fusion = result.fusion
    fusion.coarsen(factor)
    clk.lap("coarsen")
    version = int(result.scene_knowledge.get("scan_version", 0)) + 1
    grid = {"voxel_size": float(fusion.voxel_size), "nvox": [int(v) for v in fusion.nvox],
            "index_offset": [int(v) for v in fusion.index_offset]}
    res = _after_fusion(fusion, fusion.origin, fusion.nvox, result.xyz, clk, class_names, class_colors, version, out_dir, object_meshes,
                        marching_cubes, python_lists, extra=grid)
    res.seconds = clk.seconds
    return res


def resample_scene(result, class_names, class_colors=None, lattice_of=None, transform=None, voxel_size=None, origin=None,
                   index_offset=None, nvox=None, min_cover=0.5, multiple=4, out_dir=None, object_meshes=True, marching_cubes=None,
                   python_lists=False):
    """A reconstruction on another lattice, in another frame: ``result.fusion.resample(...)`` -- every new voxel the trilinear blend
    of the observed old voxels around its centre (saf_volume_resample), no frame goes through the backbones again --
    and the stages behind the fusion run again on the new volume, which keeps fusing there (``extend_scene``, with poses in the
    NEW frame).  ``lattice_of`` (a ``SceneResult`` or a fusion module), ``transform`` (4 x 4 rigid ``new_from_old``),
    ``voxel_size``, ``origin``, ``index_offset`` / ``nvox``, ``min_cover`` and ``multiple`` are ``resample``'s.  Two headsets, or
    two sessions, that scanned one room in two world frames: ``resample_scene(other, class_names, lattice_of=result, transform=T)``
    with ``T`` from ``refine_pose``, then ``join_scenes(result, other, class_names)``.

    Returns a new ``SceneResult`` around ``result.fusion`` -- ``result`` itself describes a volume the module no longer holds --;
    ``origin`` and ``nvox`` are the new volume's, ``xyz`` is ``result``'s cloud taken through ``transform``,
    ``scene_knowledge["scan_version"]`` counts on from ``result``'s, ``scene_knowledge`` gains ``voxel_size``, ``nvox`` and
    ``index_offset`` of the new volume (and so does ``scene_knowledge.json``), ``seconds`` gains ``resample``.  Objects are
    discovered anew from the new labels: an object keeps no identity across a resampling (the overlap of objects across two
    lattices is not defined here)."""
    clk = _Clock()
    clk.start()
    fusion = result.fusion
    rec = fusion.resample(origin=origin, voxel_size=voxel_size, index_offset=index_offset, nvox=nvox, transform=transform,
                          lattice_of=lattice_of, min_cover=min_cover, multiple=multiple)
    clk.lap("resample")
    xyz = result.xyz
    if transform is not None and xyz is not None:
        t = torch.as_tensor(rec.transform)
        xyz = (xyz.to(torch.float64) @ t[:3, :3].T.to(xyz.device) + t[:3, 3].to(xyz.device)).to(xyz.dtype)
    version = int(result.scene_knowledge.get("scan_version", 0)) + 1
    grid = {"voxel_size": float(fusion.voxel_size), "nvox": [int(v) for v in fusion.nvox],
            "index_offset": [int(v) for v in fusion.index_offset]}
    res = _after_fusion(fusion, fusion.origin, fusion.nvox, xyz, clk, class_names, class_colors, version, out_dir, object_meshes,
                        marching_cubes, python_lists, extra=grid)
    res.seconds = clk.seconds
    return res
