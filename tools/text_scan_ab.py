"""One process = one library (SAF_LIB_PATH) = one measurement per text scan, taken the way bench.py's side_workloads takes
a9_softmax_L5_fp32_volume, a10_surgery_L63_fp32_volume and a10_surgery_L63_bf16_volume: the same volumes (256^3 x 512, seed 100),
the same text (seed 9), two warm calls, then HIP events around three calls.  Prints one JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatially_aware_ai_amd import _abi, _lib  # noqa: E402
from spatially_aware_ai_amd.clipfusion import _query_scan  # noqa: E402

device = torch.device("cuda", 0)
n, d, q, n_bg = 256 ** 3, 512, 1000, 4
g = torch.Generator(device=device).manual_seed(100)
feats16 = torch.empty((1 << 20, d), dtype=torch.float16, device=device)
for s0 in range(0, n, 1 << 20):  # (bench.py draws the fp16 volume first: the same generator state for the fp32 one)
    feats16[:] = torch.randn((1 << 20, d), generator=g, device=device).half()
del feats16
text = torch.randn((n_bg + q, d), generator=torch.Generator().manual_seed(9))
text = (text / text.norm(dim=-1, keepdim=True)).to(device)
f32 = torch.empty((n, d), dtype=torch.float32, device=device)
for s0 in range(0, n, 1 << 20):
    f32[s0:s0 + (1 << 20)] = torch.randn((min(1 << 20, n - s0), d), generator=g, device=device)
b16 = torch.empty((n, d), dtype=torch.bfloat16, device=device)
for s0 in range(0, n, 1 << 20):
    b16[s0:s0 + (1 << 20)] = f32[s0:s0 + (1 << 20)].to(torch.bfloat16)
res = {"lib": _lib.LIB_PATH, "label": sys.argv[1] if len(sys.argv) > 1 else ""}
for name, nl, epi, scale, vol_t in (("a9_softmax_L5_fp32_volume", 5, _abi.SAF_Q_SOFTMAX, 100.0, f32),
                                    ("a10_surgery_L63_fp32_volume", 63, _abi.SAF_Q_SURGERY, 1.0, f32),
                                    ("a10_surgery_L63_bf16_volume", 63, _abi.SAF_Q_SURGERY, 1.0, b16)):
    t = text[:nl]
    last = epi == _abi.SAF_Q_SOFTMAX
    hold = {}
    fn = lambda: hold.__setitem__("o", _query_scan(vol_t, t, epi, scale=scale, normalize=True, last_only=last))  # noqa: E731
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    fn()
    fn()
    e1.record()
    torch.cuda.synchronize()
    res[name] = round(e0.elapsed_time(e1) / 3, 4)
    os.environ["SAF_Q_SPLIT"] = "0"  # the exact-fp32 matrix scan (bench.py: exact_fp32_mfma_ms)
    try:
        fn()
        torch.cuda.synchronize()
        e0.record()
        fn()
        fn()
        e1.record()
        torch.cuda.synchronize()
        res[name + "_exact"] = round(e0.elapsed_time(e1) / 2, 4)
    finally:
        del os.environ["SAF_Q_SPLIT"]
    hold.clear()
print(json.dumps(res), flush=True)
