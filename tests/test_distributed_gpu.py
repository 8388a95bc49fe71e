"""The multi-rank job ON THE DEVICE at world 2 and 4: several ranks on the one GPU a test run sees, backend gloo with device
tensors (gloo implements every collective the merge uses: reduce_scatter_tensor, all_gather_into_tensor, all_reduce,
all_to_all_single with uneven splits, reduce, broadcast, all_gather), against the CPU oracle fusing EVERY frame in one
process (running mean).  What runs on the device here and nowhere else in the suite at more than one rank:
``merge_volumes`` (dense, packed: the HIP branch of ``_reduce_scatter_packed``, all_reduce, gather), ``fuse_merge_pipelined``
(slabs, ramp, a communication stream of its own, the recycled path), ``gather_shards``, ``means_to_sums``, ``finalize_sums``,
``query_sharded`` with the HIP scan, the queue's ``flush()`` in front of a merge, the lazy ``reset()`` between two jobs, ranks
without frames.  RCCL itself runs only in tests/test_nccl_world1.py (one device cannot host two RCCL ranks).

Ranks are fresh interpreters (tests/dist_gpu_child.py), one spawn at a time, at most 4 ranks + pytest on the GPU.  The parent
polls them: the first rank that exits non-zero, or the 300 s hang guard, ends the others and fails the test with the tail of
every rank's stderr.  Workloads: tests/dist_workloads.py; that the reference alone keeps the elementwise bar on them is the CPU
companion's business (test_sharded_oracle_sums_stay_inside_the_bar_of_the_gpu_workloads).

Bars (tests/test_distributed_cpu.py): weight, tsdf_weight, labels_one_hot, stripes, counters exact; clip_feat and rgb rtol 1e-4,
atol 1e-6; tsdf rtol 1e-4, atol 2e-6.  Scan outputs: test_wide_scan_v2_scores_and_epilogues' for fp16 rows.

Wall time of this module on an MI355X: 121 s for its 16 tests (summed inside one run of the whole ``-m gpu`` suite, which took
301 s); the largest single spawn 19 s (the pipelined case at world 4), far below the 300 s guard."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import dist_workloads as wl
from spatially_aware_ai_amd import distributed as sdist

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "dist_gpu_child.py")
SPAWN_LIMIT_S = 300  # a hang guard (the value tests/test_nccl_world1.py uses), not a measurement
_REF = {}


def _spawn(scenario, world, out_dir):
    """Start ``world`` ranks of one scenario, wait for all of them; trouble on one ends the others.  Returns the ranks' results."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    env.pop("SAF_MERGE_SPARSE", None)
    env.pop("SAF_WIN_FORM", None)
    procs, logs = [], []
    for r in range(world):
        err = open(os.path.join(out_dir, f"rank{r}.err"), "w+")
        logs.append(err)
        procs.append(subprocess.Popen([sys.executable, CHILD, scenario, str(r), str(world), str(port), str(out_dir)], env=env,
                                      stdout=err, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL))
    t0, why = time.monotonic(), None
    try:
        while why is None:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes):
                why = f"rank exit codes {codes}"
            elif all(c == 0 for c in codes):
                break
            elif time.monotonic() - t0 > SPAWN_LIMIT_S:
                why = f"no end after {SPAWN_LIMIT_S} s (exit codes {codes})"
            else:
                time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    tails = []
    for r, f in enumerate(logs):
        f.seek(0)
        tails.append(f"--- rank {r} ---\n" + f.read()[-3000:])
        f.close()
    if why is not None:
        pytest.fail(f"{scenario} at world {world}: {why}\n" + "\n".join(tails), pytrace=False)
    return [dict(np.load(os.path.join(out_dir, f"rank{r}.npz"))) for r in range(world)]


def _ref(oracle, name, world, extra=False):
    key = (name, world if name == "W3" else 0, extra)
    if key not in _REF:
        s = wl.spec(name, world)
        frames = wl.frames_of(s) + (wl.extra_frame(s) if extra else [])
        _REF[key] = wl.reference(oracle, s, frames)
    return _REF[key]


def _close(got, want, name, what):
    worst = wl.elementwise_excess(got, want, name)
    print(f"{what} {name}: worst error over the elementwise bar {worst:.3g}")
    assert worst <= 1.0, f"{what}: {name} misses the elementwise bar by a factor {worst:.3g}"


def _check_job(res, job, ref, world, plan=None, whole=False, weight_everywhere=True):
    """One job's results on every rank against the reference: stripes as planned, every voxel finalised exactly once (or on
    every rank: ``whole``), integer tensors exact, float tensors within the bar; all ranks bit-identical when whole."""
    n = ref["weight"].shape[0]
    covered = np.zeros(n, dtype=np.int32)
    names = [k for k in wl.FLOAT_TENSORS + wl.INT_TENSORS if k in ref]
    for r in range(world):
        g = res[r]
        stripes = [tuple(int(v) for v in st) for st in g[f"{job}/stripes"]]
        if whole:
            assert stripes == ([(0, n)] if plan is None else plan(r)), (job, r, stripes)
            for k in names:
                assert np.array_equal(g[f"{job}/sha/{k}"], res[0][f"{job}/sha/{k}"]), f"{job}: {k} of rank {r} differs from rank 0's"
        elif plan is not None:
            assert stripes == plan(r), (job, r, stripes[:4], plan(r)[:4])
        if weight_everywhere:
            assert np.array_equal(g[f"{job}/weight_all"], ref["weight"]), f"{job}: weight of rank {r} is not the job's total on every row"
        for first, count in stripes:
            covered[first:first + count] += 1
        if whole and r > 0:
            continue
        rows = np.concatenate([np.arange(f, f + c) for f, c in stripes])
        for k in wl.INT_TENSORS:
            if k in ref:
                assert np.array_equal(g[f"{job}/{k}"], ref[k][rows]), f"{job}: {k} on rank {r}"
        for k in wl.FLOAT_TENSORS:
            _close(g[f"{job}/{k}"], ref[k][rows], k, f"{job} rank {r}")
    assert (covered == (world if whole else 1)).all(), f"{job}: every voxel must be finalised by exactly the ranks that own it"


def _merge_plan(name, world, piece_bytes="workload"):
    s = wl.spec(name, world)
    plan = wl.plan_of(s, world, piece_bytes)
    return lambda r: sdist.stripes_of_rank(plan, r, world)


def _slab_plan(name, world, n_slabs, ramp):
    """The stripes ``fuse_merge_pipelined`` leaves: per slab, what ``merge_slab_sums`` plans (slab after slab, not merged
    across slabs)."""
    s = wl.spec(name, world)
    nx, ny, nz = s["nvox"]
    rows = sdist.piece_rows_for(wl.row_bytes(s), world, s["piece_bytes"])

    def of_rank(r):
        out = []
        for x0, cnt in sdist.slab_bounds(nx, n_slabs, ramp=ramp):
            out += sdist.stripes_of_rank(sdist.stripe_plan(cnt * ny * nz, world, rows, x0 * ny * nz), r, world)
        return out

    return of_rank


WORLDS = [2, 4]


@pytest.mark.parametrize("world", WORLDS)
def test_dense_merge_gather_and_one_more_frame(tmp_path, oracle, world):
    """Case 1 and the bookkeeping of case 10.  merge_volumes(reduce_scatter, sparse=0, gather=False) on W1 (every shard on the
    windowed path): stripes as planned, each voxel finalised once, values as the reference.  The striped volume refuses
    integrate_features, merge_volumes and fuse_merge_pipelined (SafError); gather_shards makes it whole on every rank
    (bit-identical), and one more frame fused by every rank equals the oracle fed that frame; a bf16 volume is refused by
    both merges before any collective (all ranks raise, nobody hangs)."""
    res = _spawn("dense", world, tmp_path)
    ref = _ref(oracle, "W1", world)
    assert all(int(g["dense/fuse_stats"][0]) > 0 for g in res), "a shard did not take the windowed path"
    plan = _merge_plan("W1", world)
    assert all(len(plan(r)) >= 3 for r in range(world))
    _check_job(res, "dense", ref, world, plan=plan)
    s = wl.spec("W1", world)
    for r, g in enumerate(res):
        assert int(g["dense/stats"][2]) > 0
        assert not bool(g["dense/shard_stripes_none"]) and bool(g["gathered/shard_stripes_none"])
        for k in ("integrate_refused", "merge_refused", "pipelined_refused", "bf16_merge_refused", "bf16_pipelined_refused"):
            assert bool(g[f"book/{k}"]), (k, r)
    _check_job(res, "gathered", ref, world, whole=True)
    _check_job(res, "extra", _ref(oracle, "W1", world, extra=True), world, whole=True)


@pytest.mark.parametrize("world", WORLDS)
def test_whole_volume_merges_and_a_running_mean_volume(tmp_path, oracle, world):
    """Case 2: all_reduce and reduce_scatter + gather leave the whole merged volume on every rank, bit-identical across the
    ranks.  Case 7: a volume fused in SAF_RUNNING_MEAN (W2, label volume) enters merge_volumes, which converts it with
    means_to_sums itself -- the same reference."""
    res = _spawn("whole", world, tmp_path)
    ref = _ref(oracle, "W1", world)
    _check_job(res, "all_reduce", ref, world, whole=True)
    _check_job(res, "rs_gather", ref, world, whole=True)
    _check_job(res, "mean_W2", _ref(oracle, "W2", world), world, plan=_merge_plan("W2", world))


@pytest.mark.parametrize("world", WORLDS)
def test_packed_route_on_the_device(tmp_path, oracle, world):
    """Case 3, W2: the HIP branch of the packed route (scan of the touched rows, pinned split sizes, pack, all_to_all_single,
    add) with sparse = 1.0 (every piece packed), 0.3 (some), None (library default: probe, then 0.5) and ranks whose
    SAF_MERGE_SPARSE differ (they agree on dense).  touched_rows is the reference's count of weight > 0; a piece is wholly
    untouched; with 1.0 some rank receives nothing in a piece in which another receives rows.  weight is the job's total on
    every row of every rank.  Packed against dense: integer tensors identical, floats within the bar; packed twice: bit-identical."""
    res = _spawn("packed", world, tmp_path)
    ref = _ref(oracle, "W2", world)
    s = wl.spec("W2", world)
    plan = wl.plan_of(s, world)
    touched = int((ref["weight"] > 0).sum())
    of_rank = _merge_plan("W2", world)
    for job in ("dense", "p10", "p10_again", "p03", "default", "mismatch"):
        _check_job(res, job, ref, world, plan=of_rank)
    for r, g in enumerate(res):
        lm = {job: dict(zip(("pieces", "packed", "rows", "touched_rows"), g[f"{job}/last_merge"].tolist())) for job in
              ("dense", "p10", "p03", "default", "mismatch")}
        assert all(v["pieces"] == len(plan) >= 3 and v["rows"] == ref["weight"].shape[0] for v in lm.values())
        assert lm["dense"]["packed"] == 0 and lm["mismatch"]["packed"] == 0
        assert lm["p10"]["packed"] == len(plan) and 0 < lm["p03"]["packed"] < len(plan) and lm["default"]["packed"] >= 1
        assert lm["p10"]["touched_rows"] == lm["p03"]["touched_rows"] == lm["default"]["touched_rows"] == touched
        offs = g["p10/offs"]
        counts = np.diff(offs[:, :world + 1], axis=1)  # (the last column: the end of the piece, a tail of < world rows included)
        want = np.array([[int((ref["weight"][f + k * c:f + (k + 1) * c] > 0).sum()) for k in range(world)] for f, _, c in plan])
        print(f"rank {r}: touched rows per (piece, rank)\n{counts}")
        assert np.array_equal(counts, want), "the scan kernel's positions disagree with the reference's touched rows"
        assert (counts.sum(1) == 0).any() and ((counts == 0).any(1) & (counts > 0).any(1)).any()
        for k in wl.INT_TENSORS + wl.FLOAT_TENSORS:
            assert np.array_equal(g[f"p10/{k}"], g[f"p10_again/{k}"]), f"two packed runs differ in {k}"
        for k in wl.INT_TENSORS:
            assert np.array_equal(g[f"p10/{k}"], g[f"dense/{k}"]) and np.array_equal(g[f"p03/{k}"], g[f"dense/{k}"]), k
        for k in wl.FLOAT_TENSORS:
            _close(g[f"p10/{k}"], g[f"dense/{k}"], k, f"packed against dense, rank {r}")


PIPE_JOBS = (("s4_ramp_own_dense", "W1", 4, True), ("s4_flat_main_packed", "W1", 4, False), ("s4_ramp_own_allreduce", "W1", 4, True),
             ("s1_own_dense", "W1", 1, False), ("s4_aligned_main_dense", "W1a", 4, False), ("s4_seem_own_packed", "W2", 4, True),
             ("s1_rows_own_packed", "W1", 1, True))


@pytest.mark.parametrize("world", WORLDS)
def test_pipelined_fuse_and_merge(tmp_path, oracle, world):
    """Case 4: fuse_merge_pipelined with 1 and 4 slabs (unaligned on 41 planes, aligned on 64), ramp on and off, a communication
    stream of its own and none, reduce_scatter dense and packed, all_reduce; several pieces per slab (``_PIECE_BYTES``).  The
    buffers are read on the caller's stream right behind the call, with no synchronisation in between.  With SAF_WIN_FORM=rows
    (frame-ordered fusion), one slab and the packed route the result is bit for bit merge_volumes' for the same job and plan."""
    res = _spawn("pipelined", world, tmp_path)
    for job, name, n_slabs, ramp in PIPE_JOBS:
        ref = _ref(oracle, name, world)
        if "allreduce" in job:  # every slab is complete on every rank: the stripes are the slabs
            ny_nz = wl.spec(name, world)["nvox"][1] * wl.spec(name, world)["nvox"][2]
            slabs = [(x0 * ny_nz, cnt * ny_nz) for x0, cnt in sdist.slab_bounds(wl.spec(name, world)["nvox"][0], n_slabs, ramp=ramp)]
            _check_job(res, job, ref, world, whole=True, plan=lambda r: slabs)
            continue
        of_rank = _slab_plan(name, world, n_slabs, ramp)
        _check_job(res, job, ref, world, plan=of_rank)
        for g in res:
            assert len(g[f"{job}/plans"]) >= 2 * n_slabs or name == "W2", "a slab in one piece"
            if name != "W2":
                assert int(g[f"{job}/window_rows"][0]) > 0
    assert all(x % 16 == 0 and c % 16 == 0 for x, c in sdist.slab_bounds(64, 4)) and sdist.slab_bounds(41, 4)[0][1] % 16 != 0
    _check_job(res, "s1_rows_own_packed_mv", _ref(oracle, "W1", world), world, plan=_merge_plan("W1", world))
    for r, g in enumerate(res):
        assert np.array_equal(g["s1_rows_own_packed/stripes"], g["s1_rows_own_packed_mv/stripes"])
        for k in ("clip_feat", "rgb", "tsdf", "weight", "tsdf_weight"):
            assert np.array_equal(g[f"s1_rows_own_packed/{k}"], g[f"s1_rows_own_packed_mv/{k}"]), f"rank {r}: {k} differs bit for bit"


@pytest.mark.parametrize("world", WORLDS)
def test_two_jobs_in_one_process(tmp_path, oracle, world):
    """Case 5: job A, reset(accum_mode=SAF_SUM) (lazy), job B with other poses in the same module -- through merge_volumes
    (packed), then A again behind B and B again behind A through fuse_merge_pipelined's recycled path.  Every result equals the
    oracle's for that job alone, and after the gather every clip_feat row whose weight is 0 is exactly zero: nothing of the
    job before survives."""
    res = _spawn("two_jobs", world, tmp_path)
    a, b = _ref(oracle, "W1", world), _ref(oracle, "W1B", world)
    _check_job(res, "A_merge", a, world, plan=_merge_plan("W1", world))
    _check_job(res, "B_merge", b, world, plan=_merge_plan("W1", world))
    _check_job(res, "B_merge_whole", b, world, whole=True)
    _check_job(res, "A_pipe", a, world, plan=_slab_plan("W1", world, 4, True))
    _check_job(res, "A_pipe_whole", a, world, whole=True)
    _check_job(res, "B_pipe", b, world, plan=_slab_plan("W1", world, 4, False))
    _check_job(res, "B_pipe_whole", b, world, whole=True)
    assert not any(bool(g["A_pipe/stale_after"]) for g in res)
    for job, ref in (("B_merge_whole", b), ("A_pipe_whole", a), ("B_pipe_whole", b)):
        zero = ref["weight"] == 0
        assert zero.sum() > 100 and not res[0][f"{job}/clip_feat"][zero].any(), f"{job}: a row no frame of this job touched is not zero"


@pytest.mark.parametrize("world", WORLDS)
def test_queued_frames_enter_the_merge(tmp_path, oracle, world):
    """Case 6, the reference's call pattern: one frame per integrate_features call (queue + streaming session), the volume
    never read, merge_volumes called directly -- its flush() must bring in every queued frame."""
    res = _spawn("queue", world, tmp_path)
    s = wl.spec("W1", world)
    assert any(int(g["queue/pending_before"][1]) for g in res), "nothing was queued in front of the merge: the case tests nothing"
    assert sum(int(g["queue/stats"][0]) for g in res) == s["n_frames"]
    _check_job(res, "queue", _ref(oracle, "W1", world), world, plan=_merge_plan("W1", world))


@pytest.mark.parametrize("world", WORLDS)
def test_ranks_without_frames(tmp_path, oracle, world):
    """Case 8, W3: world - 1 frames, the last rank has none.  It still joins every collective of merge_volumes (dense, packed),
    of gather_shards and of fuse_merge_pipelined (n_frames = 0) and ends with the right stripes."""
    res = _spawn("few_frames", world, tmp_path)
    assert int(res[world - 1]["few/my_frames"][0]) == 0 and int(res[0]["few/my_frames"][0]) == 1
    ref = _ref(oracle, "W3", world)
    _check_job(res, "few_dense", ref, world, plan=_merge_plan("W3", world))
    _check_job(res, "few_packed", ref, world, plan=_merge_plan("W3", world))
    _check_job(res, "few_extra", _ref(oracle, "W3", world, extra=True), world, whole=True)
    _check_job(res, "few_pipe_dense", ref, world, plan=_slab_plan("W3", world, 4, True))
    _check_job(res, "few_pipe_packed", ref, world, plan=_slab_plan("W3", world, 4, False))
    assert int(res[0]["few_packed/last_merge"][3]) == int((ref["weight"] > 0).sum())


def _query_text(dim):
    text = torch.randn(24, dim, generator=torch.Generator().manual_seed(5))
    text = text / text.norm(dim=-1, keepdim=True)
    text[3] = text[11]
    v = torch.randn(dim, generator=torch.Generator().manual_seed(77))
    text[7] = v / v.norm()
    return text, v


@pytest.mark.parametrize("world", WORLDS)
def test_sharded_query_with_the_hip_scan(tmp_path, oracle, world):
    """Case 9: query_sharded with the HIP scan (fp16 shard copies) over the striped volume merge_volumes leaves (several
    stripes per rank) and over a whole volume (voxel_shard split): query_max, row_argmax (gathered and local), scores,
    vs_background; 24 queries, two of them identical, and two identical feature rows in stripes of different ranks.  Reference:
    oracle.wide_scan(round_to=float16) over the merged reference volume; values within test_wide_scan_v2_scores_and_epilogues'
    tolerances, the picked query / voxel has the maximal score within 3e-5, of tied rows the smaller voxel index wins across
    ranks, of tied queries the first.  Asked once before a one-piece merge and again after it on the same module, the second
    answer is the merged volume's (shard_features_16's key saw no change: fixed with a merge counter in the key)."""
    res = _spawn("query", world, tmp_path)
    s = wl.spec("W1", world)
    ref = _ref(oracle, "W1", world)
    text, v = _query_text(s["dim"])
    f16 = torch.float16
    n, q = ref["weight"].shape[0], text.shape[0]

    def check_reductions(job, feats, stripes_of):
        want = oracle.wide_scan(feats, text, "scores", round_to=f16)
        wv, wr = oracle.wide_scan(feats, text, "query_max", round_to=f16)
        widx, wval = oracle.wide_scan(feats, text, "row_argmax", round_to=f16)
        for r, g in enumerate(res):
            qv, qr = torch.from_numpy(g[f"{job}/query_max_0"]), torch.from_numpy(g[f"{job}/query_max_1"])
            assert np.array_equal(g[f"{job}/query_max_0"], res[0][f"{job}/query_max_0"]) and np.array_equal(g[f"{job}/query_max_1"], res[0][f"{job}/query_max_1"])
            assert (qv - wv).abs().max().item() <= 3e-5 and bool(((qr >= 0) & (qr < n)).all())
            assert (want[qr, torch.arange(q)] - wv).abs().max().item() <= 3e-5, f"{job}: query_max picked a voxel that is not the best"
            assert (qr == wr).float().mean().item() > 0.99
            idx, val = torch.from_numpy(g[f"{job}/row_argmax_0"]).long(), torch.from_numpy(g[f"{job}/row_argmax_1"])
            assert idx.shape == (n,) and (val - wval).abs().max().item() <= 3e-5
            assert (want[torch.arange(n), idx] - wval).abs().max().item() <= 3e-5, f"{job}: row_argmax picked a query that is not the best"
            assert (idx == widx).float().mean().item() > 0.999 and not bool((idx == 11).any()), "of two tied queries the first must win"
            if f"{job}/row_argmax_local_0" in g:
                rows = torch.cat([torch.arange(f, f + c) for f, c in stripes_of(r)])
                assert np.array_equal(g[f"{job}/row_argmax_local_0"], g[f"{job}/row_argmax_0"][rows.numpy()])
                assert np.array_equal(g[f"{job}/row_argmax_local_1"], g[f"{job}/row_argmax_1"][rows.numpy()])
                sc = torch.from_numpy(g[f"{job}/scores_0"])
                assert sc.shape == (rows.numel(), q) and (sc - want[rows]).abs().max().item() <= 1e-3
        return want, wv, wr

    # (a) before and after a merge in one piece: stripes == voxel_shard, the cache key's other fields unchanged
    for r, g in enumerate(res):
        assert [tuple(x) for x in g["after/stripes"].tolist()] == [sdist.voxel_shard(n, r, world)]
        assert not np.array_equal(g["before/query_max_0"], g["after/query_max_0"]), "the merge changed nothing?"
    check_reductions("after", torch.from_numpy(ref["clip_feat"]), None)
    # (b) striped, with the planted rows
    lo, hi = (int(x) for x in res[0]["striped/planted"])
    plan = wl.plan_of(s, world)
    owner = lambda row: next(r for r in range(world) if any(f <= row < f + c for f, c in sdist.stripes_of_rank(plan, r, world)))
    assert owner(lo) == 0 and owner(hi) == world - 1 and lo < hi
    feats = torch.from_numpy(ref["clip_feat"]).clone()
    feats[lo] = v
    feats[hi] = v
    of_rank = _merge_plan("W1", world)
    for r, g in enumerate(res):
        assert len(of_rank(r)) >= 3 and [tuple(x) for x in g["striped/stripes"].tolist()] == of_rank(r)
        rows = np.concatenate([np.arange(f, f + c) for f, c in of_rank(r)])
        _close(g["striped/clip_feat"], feats.numpy()[rows], "clip_feat", f"striped rank {r}")
    want, wv, wr = check_reductions("striped", feats, of_rank)
    assert int(wr[7]) == lo
    for r, g in enumerate(res):
        assert int(g["striped/query_max_1"][7]) == lo, "of two tied rows on different ranks the smaller voxel index must win"
        rows = torch.cat([torch.arange(f, f + c) for f, c in of_rank(r)])
        wb = oracle.wide_scan(feats[rows], text, "vs_background", scale=100.0, n_background=4, round_to=f16)
        gb = torch.from_numpy(g["striped/vs_background_0"])
        assert gb.shape == (rows.numel(), q - 4) and (gb - wb).abs().max().item() <= 2e-3
    # (c) the gathered volume, split by voxel_shard
    check_reductions("whole", feats, lambda r: [sdist.voxel_shard(n, r, world)])
    for g in res:
        assert int(g["whole/query_max_1"][7]) == lo
