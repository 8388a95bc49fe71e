"""256^3 x 512, 512 frames (640 x 480, depth A, the headline's shapes): fuse rate of an fp16 volume beside a bf16 one on one box,
and the float -> half pass that config 5 no longer needs.  Usage: python tools/probe_fp16_volume.py [out.json]
(profiles/r07/fp16_volume.json is its output)."""
import json, os, sys, time
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatially_aware_ai_amd import ClipFusion
from spatially_aware_ai_amd import synthetic as syn
from spatially_aware_ai_amd import distributed as D

REPEATS = 3
W, H, DIM, NF, NV = 640, 480, 512, 512, 256


class FakeClip:
    feature_dim = DIM


def ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


npy, npx = syn.feature_map_shape(W, H)
grid = syn.make_grid(NV)
t0 = time.time()
frames = syn.make_frames(2024, NF, width=W, height=H, feat_dim=DIM, npy=npy, npx=npx, depth_kind="A")
cat = lambda k: torch.cat([f[k] for f in frames]).cuda()
args = [cat(k) for k in ("depth", "rgb", "pose", "K", "feat")]
del frames
print("frames ready", round(time.time() - t0, 1), "s", flush=True)

out = {"device": torch.cuda.get_device_name(0), "grid": NV, "feat_dim": DIM, "frames": NF,
       "image": [W, H], "repeats": REPEATS, "fuse": {}}
mods = {}
for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
    mods[name] = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, FakeClip(), None, 10, 10,
                            keep_xyz_world=False, feat_dtype=dt, defer_frames=False, device="cuda").cuda()
    out["fuse"][name] = {"ms": []}
for rep in range(REPEATS + 1):  # the first round is the warm-up
    for name in (("bf16", "fp16") if rep % 2 == 0 else ("fp16", "bf16")):
        fz = mods[name]
        fz.reset()
        t = ms(lambda: fz.integrate_features(*args))
        if rep > 0:
            out["fuse"][name]["ms"].append(round(t, 3))
        print(rep, name, round(t, 2), "ms", fz.stats()["window_form"], flush=True)
for name in mods:
    v = sorted(out["fuse"][name]["ms"])
    out["fuse"][name]["frames_per_s"] = [round(NF / (x / 1e3), 1) for x in out["fuse"][name]["ms"]]
    out["fuse"][name]["median_frames_per_s"] = round(NF / (v[len(v) // 2] / 1e3), 1)
    out["fuse"][name]["window_form"] = mods[name].stats()["window_form"]
    out["fuse"][name]["window_rows"] = mods[name].stats()["window_rows"]
out["fuse"]["fp16_over_bf16"] = round(out["fuse"]["fp16"]["median_frames_per_s"] / out["fuse"]["bf16"]["median_frames_per_s"], 4)

# the pass an fp16 volume makes unnecessary: the 16-bit copy of the rows the wide scan reads (distributed.shard_features_16)
fz16 = mods["fp16"]
n = fz16.clip_feat.shape[0]
view = D.shard_features_16(fz16, 0, n, torch.float16)
out["convert"] = {"fp16_volume": {"same_buffer": view.data_ptr() == fz16.clip_feat.data_ptr(), "ms": 0.0, "bytes": 0}}
del mods["bf16"]
torch.cuda.empty_cache()
f32 = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, False, FakeClip(), None, 10, 10,
                 keep_xyz_world=False, feat_dtype=torch.float32, defer_frames=False, device="cuda").cuda()
f32.integrate_features(*[a[:128] for a in args])
times = []
for rep in range(REPEATS + 1):
    f32.__dict__["_shard16"] = None
    t = ms(lambda: D.shard_features_16(f32, 0, n, torch.float16))
    if rep > 0:
        times.append(round(t, 3))
    print("float -> half", round(t, 2), "ms", flush=True)
nbytes = n * DIM * (4 + 2)
out["convert"]["f32_volume_to_half"] = {"ms": times, "bytes_read": n * DIM * 4, "bytes_written": n * DIM * 2,
                                        "resident_copy_bytes": n * DIM * 2,
                                        "GBps": [round(nbytes / (t / 1e3) / 1e9, 1) for t in times]}
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
print(json.dumps(out))
