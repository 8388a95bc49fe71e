"""The workloads of the multi-rank tests, shared by the CPU companion (tests/test_distributed_cpu.py), the GPU test
(tests/test_distributed_gpu.py) and the rank processes it starts (tests/dist_gpu_child.py): the same seeded frames, grids and
piece sizes everywhere.  No test in here.

  W1   ClipFusion, D = 512 f32, 41 x 35 x 33 = 47355 voxels (odd: no multiple of the world size nor of 64; 41 x-planes: slabs
       cannot be aligned to 16), incoherent depth (kind A), 96 frames -- 24 per rank at world 4, 48 at world 2: every shard
       takes the windowed path.  Job B (two jobs in one process): 64 other frames from a nearer camera sphere.
  W1a  the same on 64 x 29 x 27 (nx a multiple of 16 and >= 64: four aligned slabs of 16 planes).
  W2   ClipSeemFusion (label histogram [N, 143], bilinear rgb), D = 64, the coherent scene (kind B) in a 4.2 m grid -- wider
       than the 2.4 m room --, truncation of one voxel, 41 x 29 x 25 = 29725 voxels in pieces of 2400 rows: 13 pieces, the last
       one ragged (925 rows) with a tail of one row at world 2 and 4.
  W3   W1's grid with world - 1 frames: the last rank has none.
"""
import numpy as np
import torch

from spatially_aware_ai_amd import _abi
from spatially_aware_ai_amd import distributed as sdist
from spatially_aware_ai_amd import synthetic as syn

IMG_W, IMG_H = 64, 48
N_CLASSES = 143
FLOAT_TENSORS = ("clip_feat", "rgb", "tsdf")
INT_TENSORS = ("weight", "tsdf_weight", "labels_one_hot")

WORKLOADS = {
    "W1": dict(nvox=(41, 35, 33), side=2.56, trunc_vox=3.0, dim=512, seem=False, depth_kind="A", seed=1101, n_frames=96,
               piece_bytes=512 * 4 * 5000),
    "W1B": dict(nvox=(41, 35, 33), side=2.56, trunc_vox=3.0, dim=512, seem=False, depth_kind="A", seed=2202, n_frames=64,
                radius=1.9, piece_bytes=512 * 4 * 5000),
    "W1a": dict(nvox=(64, 29, 27), side=2.56, trunc_vox=3.0, dim=512, seem=False, depth_kind="A", seed=1101, n_frames=96,
                piece_bytes=512 * 4 * 5000),
    "W2": dict(nvox=(41, 29, 25), side=4.2, trunc_vox=1.0, dim=64, seem=True, depth_kind="B", seed=321, n_frames=12,
               piece_bytes=N_CLASSES * 4 * 2400),
    "W3": dict(nvox=(41, 35, 33), side=2.56, trunc_vox=3.0, dim=512, seem=False, depth_kind="A", seed=3303, n_frames=None,
               piece_bytes=512 * 4 * 5000),
}
EXTRA_SEED = 4404  # the one more frame every rank fuses after gather_shards


def spec(name, world):
    s = dict(WORKLOADS[name], name=name)
    if s["n_frames"] is None:
        s["n_frames"] = world - 1
    return s


def grid_of(s):
    return syn.make_grid(s["nvox"], side=s["side"], trunc_vox=s["trunc_vox"])


def frames_of(s, seed=None, n_frames=None):
    npy, npx = syn.feature_map_shape(IMG_W, IMG_H)
    kw = {"radius": s["radius"]} if "radius" in s else {}
    return syn.make_frames(s["seed"] if seed is None else seed, s["n_frames"] if n_frames is None else n_frames, width=IMG_W,
                           height=IMG_H, feat_dim=s["dim"], npy=npy, npx=npx, depth_kind=s["depth_kind"], **kw)


def extra_frame(s):
    return frames_of(s, seed=EXTRA_SEED, n_frames=1)


def row_bytes(s):
    return 4 * max(s["dim"], N_CLASSES if s["seem"] else 0)


def plan_of(s, world, piece_bytes="workload"):
    """The stripe plan ``merge_volumes`` makes for the workload's volume."""
    n = int(np.prod(s["nvox"]))
    pb = s["piece_bytes"] if piece_bytes == "workload" else piece_bytes
    return sdist.stripe_plan(n, world, sdist.piece_rows_for(row_bytes(s), world, pb))


def oracle_volume(O, s, accum=_abi.SAF_RUNNING_MEAN):
    g = grid_of(s)
    return O.OracleVolume(g.origin, g.voxel_size, g.nvox, g.trunc, s["dim"], N_CLASSES if s["seem"] else 0, accum)


def oracle_fuse(vol, frames, seem):
    for f in frames:
        vol.integrate(f["depth"], f["rgb"], f["pose"], f["K"], f["feat"], [f["labels"].float()] if seem else None, rgb_bilinear=seem)
    return vol


def tensors_of(vol):
    names = ("clip_feat", "rgb", "tsdf", "weight", "tsdf_weight") + (("labels_one_hot",) if vol.labels_one_hot is not None else ())
    return {k: getattr(vol, k).numpy() for k in names}


def reference(O, s, frames):
    """What one process fusing every frame holds (running mean), as numpy arrays."""
    return tensors_of(oracle_fuse(oracle_volume(O, s), frames, s["seem"]))


def elementwise_excess(got, want, name):
    """The largest |got - want| / (atol + rtol |want|) under the elementwise bar of tests/test_distributed_cpu.py: <= 1 passes."""
    atol = 2e-6 if name == "tsdf" else 1e-6
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / (atol + 1e-4 * np.abs(want))).max())
