"""One rank of tests/test_distributed_gpu.py: ``python dist_gpu_child.py <scenario> <rank> <world> <port> <out dir>``.

A fresh interpreter per rank (the pytest process holds the GPU: never fork, never exec from it).  Every rank opens GPU 0 and
joins a gloo group -- several ranks on ONE device; gloo carries device tensors through host memory and implements every
collective the merge uses.  A scenario is a list of jobs on the workloads of tests/dist_workloads.py; what a job leaves on
this rank goes to ``rank<r>.npz`` (keys ``<job>/<name>``): the stripes, the volume tensors on the stripes (a whole volume:
rank 0 stores it, every rank stores a digest), the whole ``weight``, ``stats()``, ``distributed.last_merge``.  Nothing outside
the repository is read; the parent compares with the CPU oracle."""
import hashlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dist_workloads as wl  # noqa: E402
from spatially_aware_ai_amd import ClipFusion, ClipSeemFusion, _abi  # noqa: E402
from spatially_aware_ai_amd import distributed as sd  # noqa: E402
from spatially_aware_ai_amd._lib import SafError  # noqa: E402

SCENARIO, RANK, WORLD, PORT, OUT = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
RES = {}
OFFS = []  # the touched-row positions (_Touched.offs) of every packed merge of this process, in order


class _Backbone:
    def __init__(self, dim):
        self.feature_dim = dim

    def img_inference_tiled(self, rgb, patch_size, patch_stride):
        raise RuntimeError("the tests hand the feature maps in")

    def run_on_image(self, rgb_chw):
        raise RuntimeError("the tests hand the label maps in")


class _RecordingTouched(sd._Touched):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        OFFS.append(np.asarray(self.offs, dtype=np.int64))


sd._Touched = _RecordingTouched


def build(s, feat_dtype=torch.float32):
    g = wl.grid_of(s)
    if s["seem"]:
        return ClipSeemFusion(g.origin, g.voxel_size, g.nvox, g.trunc, False, 10, 10, _Backbone(s["dim"]), _Backbone(s["dim"]),
                              keep_xyz_world=False, feat_dtype=feat_dtype).cuda()
    return ClipFusion(g.origin, g.voxel_size, g.nvox, g.trunc, False, _Backbone(s["dim"]), None, 10, 10, keep_xyz_world=False,
                      feat_dtype=feat_dtype).cuda()


def batch(frames, seem):
    """(depth, rgb, pose, K, feat, labels) of some frames on the device; labels None without a label volume."""
    cat = lambda k: torch.cat([f[k] for f in frames]).cuda()
    labs = [f["labels"].float().cuda() for f in frames] if seem else None
    return cat("depth"), cat("rgb"), cat("pose"), cat("K"), cat("feat"), labs


def my_frames(frames):
    return [frames[i] for i in sd.shard_frames(len(frames), RANK, WORLD)]


def fuse(fz, frames, seem, one_by_one=False):
    if not frames:
        return
    if one_by_one:
        for f in frames:
            fz.integrate_features(*batch([f], seem))
    else:
        fz.integrate_features(*batch(frames, seem))


def digest(a):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def record(job, fz, stripes, raw=False, stats=True):
    """``raw``: read the buffers themselves on the current stream, with no synchronisation and none of the module's own
    bookkeeping in between (the pipelined merge promises that the caller's stream is ordered behind its last collective)."""
    n = fz._buffers["tsdf"].numel()
    names = [k for k in sd.VOLUME_TENSORS if fz._buffers.get(k) is not None]
    get = (lambda k: fz._buffers[k]) if raw else (lambda k: getattr(fz, k))
    whole = sum(c for _, c in stripes) == n  # ((0, n), or slab after slab behind the pipelined all_reduce)
    got = {k: (get(k) if len(stripes) == 1 else torch.cat([get(k)[f:f + c] for f, c in stripes])).cpu().numpy() for k in names}
    RES[f"{job}/stripes"] = np.asarray(stripes, dtype=np.int64).reshape(-1, 2)
    RES[f"{job}/weight_all"] = get("weight").cpu().numpy()
    for k in names:
        if whole:
            RES[f"{job}/sha/{k}"] = digest(got[k])
        if not whole or RANK == 0:
            RES[f"{job}/{k}"] = got[k]
    RES[f"{job}/last_merge"] = np.array([sd.last_merge[k] for k in ("pieces", "packed", "rows", "touched_rows")], dtype=np.int64)
    RES[f"{job}/shard_stripes_none"] = np.array(fz._shard_stripes is None)
    if stats:
        st = fz.stats()
        RES[f"{job}/stats"] = np.array([st["frames"], st["valid"], st["window_rows"]], dtype=np.int64)


def raises_saf(fn):
    try:
        fn()
    except SafError:
        return True
    return False


def pipelined(fz, s, frames, **kw):
    """fuse_merge_pipelined on this rank's frames (none: a NULL frame array and n_frames = 0; the rank still joins every
    collective)."""
    if fz.accum_mode != _abi.SAF_SUM:  # (a volume fresh from reset(accum_mode=SAF_SUM) keeps its deferred clear: not touched)
        fz.accum_mode = _abi.SAF_SUM
    npy, npx = wl.syn.feature_map_shape(wl.IMG_W, wl.IMG_H)
    ws = fz._get_workspace(npy, npx)
    if frames:
        d, rgb, pose, k, feat, labs = batch(frames, s["seem"])
        arr, keep, _, _ = fz._make_frames(d, rgb, pose, k, feat, labs, s["seem"])
    else:
        arr, keep = None, None
    stripes = sd.fuse_merge_pipelined(fz, arr, len(frames), ws, **kw)
    return stripes, keep


# ---- scenarios ------------------------------------------------------------------------------------------------------------
def scenario_dense():
    """Case 1 (+ 10): merge_volumes, reduce_scatter, dense, striped; gather_shards; one more frame on every rank."""
    s = wl.spec("W1", WORLD)
    fz = build(s)
    fz.accum_mode = _abi.SAF_SUM
    fuse(fz, my_frames(wl.frames_of(s)), False)
    RES["dense/fuse_stats"] = np.array([fz.stats()["window_rows"]], dtype=np.int64)
    stripes = sd.merge_volumes(fz, mode="reduce_scatter", gather=False, piece_bytes=s["piece_bytes"], sparse=0)
    record("dense", fz, stripes)
    extra = wl.extra_frame(s)
    RES["book/integrate_refused"] = np.array(raises_saf(lambda: fuse(fz, extra, False)) and fz.pending_frames == 0)
    RES["book/merge_refused"] = np.array(raises_saf(lambda: sd.merge_volumes(fz)))
    npy, npx = wl.syn.feature_map_shape(wl.IMG_W, wl.IMG_H)
    RES["book/pipelined_refused"] = np.array(raises_saf(lambda: sd.fuse_merge_pipelined(fz, None, 0, fz._get_workspace(npy, npx))))
    assert sd.gather_shards(fz) == [(0, fz.tsdf.numel())]
    record("gathered", fz, [(0, fz.tsdf.numel())], stats=False)
    fuse(fz, extra, False)
    record("extra", fz, [(0, fz.tsdf.numel())], stats=False)
    del fz
    half = build(s, feat_dtype=torch.bfloat16)  # refused before any collective: every rank raises, nobody waits
    half.accum_mode = _abi.SAF_SUM
    RES["book/bf16_merge_refused"] = np.array(raises_saf(lambda: sd.merge_volumes(half)))
    RES["book/bf16_pipelined_refused"] = np.array(raises_saf(lambda: sd.fuse_merge_pipelined(half, None, 0, half._get_workspace(npy, npx))))


def scenario_whole():
    """Case 2 (whole volume on every rank) and case 7 (a running-mean volume enters the merge)."""
    s = wl.spec("W1", WORLD)
    frames = my_frames(wl.frames_of(s))
    for job, kw in (("all_reduce", dict(mode="all_reduce")), ("rs_gather", dict(mode="reduce_scatter", gather=True, sparse=0))):
        fz = build(s)
        fz.accum_mode = _abi.SAF_SUM
        fuse(fz, frames, False)
        stripes = sd.merge_volumes(fz, piece_bytes=s["piece_bytes"], **kw)
        record(job, fz, stripes)
        del fz
    for name in ("W2",):
        s = wl.spec(name, WORLD)
        fz = build(s)  # SAF_RUNNING_MEAN: merge_volumes converts with means_to_sums itself
        fuse(fz, my_frames(wl.frames_of(s)), s["seem"])
        record(f"mean_{name}", fz, sd.merge_volumes(fz, gather=False, piece_bytes=s["piece_bytes"], sparse=0))
        del fz


def scenario_packed():
    """Case 3: the packed route on the device, W2."""
    s = wl.spec("W2", WORLD)
    frames = my_frames(wl.frames_of(s))
    assert sd.probe_all_to_all(torch.device("cuda", 0)) is None
    for job, sparse, env in (("dense", 0.0, None), ("p10", 1.0, None), ("p10_again", 1.0, None), ("p03", 0.3, None),
                             ("default", None, ""), ("mismatch", None, "0" if RANK == 0 else "1.0")):
        if env in (None, ""):
            os.environ.pop("SAF_MERGE_SPARSE", None)
        else:
            os.environ["SAF_MERGE_SPARSE"] = env
        fz = build(s)
        fz.accum_mode = _abi.SAF_SUM
        fuse(fz, frames, True)
        n_offs = len(OFFS)
        stripes = sd.merge_volumes(fz, gather=False, piece_bytes=s["piece_bytes"], sparse=sparse)
        record(job, fz, stripes)
        if len(OFFS) > n_offs:
            RES[f"{job}/offs"] = OFFS[-1]
        del fz
    os.environ.pop("SAF_MERGE_SPARSE", None)


def scenario_pipelined():
    """Case 4: fuse_merge_pipelined -- slabs, ramp, communication stream, routes; the buffers are read right behind the call."""
    jobs = (("s4_ramp_own_dense", "W1", dict(n_slabs=4, ramp=True, mode="reduce_scatter", sparse=0), True, None),
            ("s4_flat_main_packed", "W1", dict(n_slabs=4, ramp=False, mode="reduce_scatter", sparse=1.0), False, None),
            ("s4_ramp_own_allreduce", "W1", dict(n_slabs=4, ramp=True, mode="all_reduce"), True, None),
            ("s1_own_dense", "W1", dict(n_slabs=1, ramp=False, mode="reduce_scatter", sparse=0), True, None),
            ("s4_aligned_main_dense", "W1a", dict(n_slabs=4, ramp=False, mode="reduce_scatter", sparse=0), False, None),
            ("s4_seem_own_packed", "W2", dict(n_slabs=4, ramp=True, mode="reduce_scatter", sparse=1.0), True, None),
            ("s1_rows_own_packed", "W1", dict(n_slabs=1, ramp=True, mode="reduce_scatter", sparse=1.0), True, "rows"))
    for job, name, kw, own, form in jobs:
        s = wl.spec(name, WORLD)
        sd._PIECE_BYTES = s["piece_bytes"]
        if form:
            os.environ["SAF_WIN_FORM"] = form
        fz = build(s)
        frames = my_frames(wl.frames_of(s))
        stripes, keep = pipelined(fz, s, frames, comm_stream=torch.cuda.Stream() if own else None, **kw)
        record(job, fz, stripes, raw=True, stats=False)
        RES[f"{job}/plans"] = np.asarray([p for plan in (fz.__dict__.get("_shard_plans") or []) for p in plan], dtype=np.int64).reshape(-1, 3)
        torch.cuda.synchronize()
        RES[f"{job}/window_rows"] = np.array([fz.stats()["window_rows"]], dtype=np.int64)
        del fz, keep
        if form:  # the same job and plan through merge_volumes, frame-ordered fusion: bit for bit the same sums
            fz = build(s)
            fz.accum_mode = _abi.SAF_SUM
            fuse(fz, frames, s["seem"])
            record(job + "_mv", fz, sd.merge_volumes(fz, gather=False, piece_bytes=s["piece_bytes"], sparse=1.0))
            del fz
            os.environ.pop("SAF_WIN_FORM", None)


def scenario_two_jobs():
    """Case 5: job A, a lazy reset, job B in the same module -- through merge_volumes, then (A again, behind B) through the
    recycled path of fuse_merge_pipelined."""
    a, b = wl.spec("W1", WORLD), wl.spec("W1B", WORLD)
    sd._PIECE_BYTES = a["piece_bytes"]
    fa, fb = my_frames(wl.frames_of(a)), my_frames(wl.frames_of(b))
    fz = build(a)
    fz.accum_mode = _abi.SAF_SUM
    fuse(fz, fa, False)
    record("A_merge", fz, sd.merge_volumes(fz, gather=False, piece_bytes=a["piece_bytes"], sparse=0))
    fz.reset(accum_mode=_abi.SAF_SUM)
    assert fz.__dict__["_feat_stale"]
    fuse(fz, fb, False)
    record("B_merge", fz, sd.merge_volumes(fz, gather=False, piece_bytes=a["piece_bytes"], sparse=1.0), stats=False)
    sd.gather_shards(fz)
    record("B_merge_whole", fz, [(0, fz.tsdf.numel())], stats=False)
    # the volume now holds job B; job A again through the pipelined merge's recycled path
    fz.reset(accum_mode=_abi.SAF_SUM)
    assert fz.__dict__["_feat_stale"]
    stripes, keep = pipelined(fz, a, fa, n_slabs=4, ramp=True, comm_stream=torch.cuda.Stream(), mode="reduce_scatter", sparse=0)
    RES["A_pipe/stale_after"] = np.array(bool(fz.__dict__["_feat_stale"]))
    record("A_pipe", fz, stripes, raw=True, stats=False)
    sd.gather_shards(fz)
    record("A_pipe_whole", fz, [(0, fz.tsdf.numel())], stats=False)
    # and B behind A, pipelined and packed
    fz.reset(accum_mode=_abi.SAF_SUM)
    stripes, keep = pipelined(fz, b, fb, n_slabs=4, ramp=False, comm_stream=None, mode="reduce_scatter", sparse=1.0)
    record("B_pipe", fz, stripes, raw=True, stats=False)
    sd.gather_shards(fz)
    record("B_pipe_whole", fz, [(0, fz.tsdf.numel())], stats=False)


def scenario_queue():
    """Case 6: one frame per integrate_features call (queue + streaming session), the volume not read, merge_volumes directly."""
    s = wl.spec("W1", WORLD)
    fz = build(s)
    fz.accum_mode = _abi.SAF_SUM
    fuse(fz, my_frames(wl.frames_of(s)), False, one_by_one=True)
    RES["queue/pending_before"] = np.array([fz.pending_frames, int(bool(fz._queue_busy()))], dtype=np.int64)
    record("queue", fz, sd.merge_volumes(fz, gather=False, piece_bytes=s["piece_bytes"], sparse=1.0))


def scenario_few_frames():
    """Case 8: fewer frames than ranks through cases 1, 3 (sparse = 1.0) and 4."""
    s = wl.spec("W3", WORLD)
    sd._PIECE_BYTES = s["piece_bytes"]
    frames = my_frames(wl.frames_of(s))
    RES["few/my_frames"] = np.array([len(frames)], dtype=np.int64)
    for job, sparse in (("few_dense", 0.0), ("few_packed", 1.0)):
        fz = build(s)
        fz.accum_mode = _abi.SAF_SUM
        fuse(fz, frames, False)
        record(job, fz, sd.merge_volumes(fz, gather=False, piece_bytes=s["piece_bytes"], sparse=sparse))
        if job == "few_dense":
            sd.gather_shards(fz)
            fuse(fz, wl.extra_frame(s), False)
            record("few_extra", fz, [(0, fz.tsdf.numel())], stats=False)
        del fz
    for job, kw, own in (("few_pipe_dense", dict(n_slabs=4, ramp=True, sparse=0), True), ("few_pipe_packed", dict(n_slabs=4, ramp=False, sparse=1.0), False)):
        fz = build(s)
        stripes, keep = pipelined(fz, s, frames, comm_stream=torch.cuda.Stream() if own else None, mode="reduce_scatter", **kw)
        record(job, fz, stripes, raw=True, stats=False)
        del fz, keep


def query_text(dim):
    text = torch.randn(24, dim, generator=torch.Generator().manual_seed(5))
    text = text / text.norm(dim=-1, keepdim=True)
    text[3] = text[11]
    return text


def planted_row(dim):
    return torch.randn(dim, generator=torch.Generator().manual_seed(77))


def scenario_query():
    """Case 9: query_sharded with the HIP scan over a striped merged volume and over a whole one; before and after a merge."""
    s = wl.spec("W1", WORLD)
    frames = my_frames(wl.frames_of(s))
    text = query_text(s["dim"]).cuda()
    text[7] = (planted_row(s["dim"]) / planted_row(s["dim"]).norm()).cuda()

    def run(job, fz, epilogues):
        for epi, kw in epilogues:
            out = sd.query_sharded(fz, text, epi, **kw)
            out = out if isinstance(out, tuple) else (out,)
            tag = epi + ("_local" if kw.get("gather") is False else "")
            for i, t in enumerate(out):
                RES[f"{job}/{tag}_{i}"] = t.float().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()

    # (a) one module, asked before and after a merge in ONE piece: the shard range, the dtype, the address and the frame
    # count are what they were -- the answer must still be the merged volume's
    fz = build(s)
    fz.accum_mode = _abi.SAF_SUM
    fuse(fz, frames, False)
    run("before", fz, [("query_max", {})])
    stripes = sd.merge_volumes(fz, gather=False, piece_bytes=None, sparse=0)
    RES["after/stripes"] = np.asarray(stripes, dtype=np.int64).reshape(-1, 2)
    run("after", fz, [("query_max", {}), ("row_argmax", {})])
    del fz
    # (b) several stripes per rank; two identical rows in stripes of different ranks
    fz = build(s)
    fz.accum_mode = _abi.SAF_SUM
    fuse(fz, frames, False)
    stripes = sd.merge_volumes(fz, gather=False, piece_bytes=s["piece_bytes"], sparse=0)
    plan = wl.plan_of(s, WORLD)
    lo, hi = sd.stripes_of_rank(plan, 0, WORLD)[1][0] + 5, sd.stripes_of_rank(plan, WORLD - 1, WORLD)[2][0] + 9
    RES["striped/planted"] = np.array([lo, hi], dtype=np.int64)
    v = planted_row(s["dim"]).cuda()
    fz.clip_feat[lo] = v
    fz.clip_feat[hi] = v
    fz.__dict__["_shard16"] = None  # (the rows were written behind the module's back)
    RES["striped/stripes"] = np.asarray(stripes, dtype=np.int64).reshape(-1, 2)
    RES["striped/clip_feat"] = torch.cat([fz.clip_feat[f:f + c] for f, c in stripes]).cpu().numpy()
    run("striped", fz, [("query_max", {}), ("row_argmax", {}), ("row_argmax", {"gather": False}), ("scores", {"out_dtype": torch.float16}),
                        ("vs_background", {"n_background": 4, "scale": 100.0, "out_dtype": torch.float16})])
    sd.gather_shards(fz)
    RES["whole/stripes"] = np.asarray([sd.voxel_shard(fz.tsdf.numel(), RANK, WORLD)], dtype=np.int64)
    run("whole", fz, [("query_max", {}), ("row_argmax", {}), ("row_argmax", {"gather": False}), ("scores", {"out_dtype": torch.float16})])


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{PORT}", world_size=WORLD, rank=RANK)
    try:
        globals()["scenario_" + SCENARIO]()
        torch.cuda.synchronize()
        np.savez(os.path.join(OUT, f"rank{RANK}.npz"), **RES)
        dist.barrier()
    finally:
        dist.destroy_process_group()
    print("RANK_OK", flush=True)


if __name__ == "__main__":
    main()
