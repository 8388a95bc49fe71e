"""Pins the tiled CLIP front-end (Clip.get_patches / Clip.img_inference_tiled,
reference clipfusion.py:789-839) against goldens produced by the reference's own code with the ViT replaced
by a stub encode_image (oracle/gen_golden.py::gen_tiled_clip).  The PyTorch restatement runs on the CPU; the
fused HIP front-end (saf_clip_tiles) is checked against the same goldens in tests/test_gpu_parity.py, and here, every pixel of
whole tiles, against the float64 statement of tests/frame_pass_reference.py (bound per pixel: E = 2^-21 * (p * R + 2 * M))."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import frame_pass_reference as R
from spatially_aware_ai_amd.clipfusion import Clip


def stub_encode_image(x):
    """Same function as oracle/gen_golden.py::stub_encode_image (test code on both sides, not reference code)."""
    x = x.float()
    return torch.cat([x.mean(dim=(2, 3)), x[:, :, 5::50, 7::50].flatten(1)[:, :9]], dim=1)


class StubBackbone(torch.nn.Module):
    class visual:
        output_dim = 12

    def __init__(self):
        super().__init__()
        self.seen = []

    def encode_image(self, x):
        self.seen.append(x.clone())
        return stub_encode_image(x)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "tiled_clip.npz"))


@pytest.mark.parametrize("case", [0, 1, 2])
def test_get_patches_and_tiled_inference_match_reference(golden, case):
    g = golden
    rgb = torch.from_numpy(g[f"c{case}_rgb"])
    ps, st = (int(v) for v in g[f"c{case}_patch"])
    bb = StubBackbone()
    clip = Clip("stub", None, backbone=bb, tokenizer=None)
    patches = clip.get_patches(rgb, ps, st)
    assert tuple(patches.shape) == tuple(int(v) for v in g[f"c{case}_patches_shape"])
    assert np.array_equal(patches[:, :, :, :, ::3, ::3].numpy(), g[f"c{case}_patches_sample"]), "tile order / content"
    for cap in (8, 1024, 5):  # the reference's cap, ours, and one that does not divide the tile count
        bb.seen.clear()
        clip.max_patch_batch_size = cap
        feats = clip.img_inference_tiled(rgb, ps, st)
        resized = torch.cat(bb.seen)
        np.testing.assert_allclose(resized[:, :, ::13, ::11].numpy(), g[f"c{case}_resized_sample"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(resized.double().sum(dim=(1, 2, 3)).numpy(), g[f"c{case}_resized_sum"], rtol=1e-6)
        assert feats.shape == g[f"c{case}_feats"].shape
        np.testing.assert_allclose(feats.numpy(), g[f"c{case}_feats"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", [0, 1])
def test_depth_scaled_tiling_matches_reference(golden, case):
    """Clip.img_inference_tiled_depthscaled (clipfusion.py:841-890; dead in the reference's drivers, the last stub of the API until
    round 4) against the reference's own output with the stub encode_image: tiles that overlap, stick out of the image and
    are missing (depth 0), batched through the backbone here and encoded one by one there."""
    g = golden
    rgb, depth, K = (torch.from_numpy(g[f"d{case}_{k}"]) for k in ("rgb", "depth", "K"))
    st = int(g[f"d{case}_stride"])
    for cap in (8, 3):
        clip = Clip("stub", None, backbone=StubBackbone(), tokenizer=None)
        clip.max_patch_batch_size = cap
        feats = clip.img_inference_tiled_depthscaled(rgb, depth, K, st)
        want = g[f"d{case}_feats"]
        assert feats.shape == want.shape
        np.testing.assert_allclose(feats.numpy(), want, rtol=1e-5, atol=1e-6)
        assert (want == 0).any() and (want != 0).any()
    # B = 2 (the reference raises there): every image as if alone
    both = clip.img_inference_tiled_depthscaled(rgb.repeat(2, 1, 1, 1), depth.repeat(2, 1, 1), K.repeat(2, 1, 1), st)
    np.testing.assert_allclose(both[1].numpy(), g[f"d{case}_feats"][0], rtol=1e-5, atol=1e-6)


def test_tile_shape_asserts_like_the_reference():
    clip = Clip("stub", None, backbone=StubBackbone(), tokenizer=None)
    with pytest.raises(AssertionError):  # (H - p) % s != 0, clipfusion.py:792-793
        clip.get_patches(torch.zeros(1, 3, 50, 64), 16, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1, 2])
def test_fused_tile_kernel_matches_reference(golden, case):
    """saf_clip_tiles (normalise + unfold + 224^2 resize in one HIP pass) against the reference's own tiles, for planar
    frames and for the channel-last frames integrate() receives (a permuted view: no copy is made)."""
    g = golden
    rgb = torch.from_numpy(g[f"c{case}_rgb"])
    ps, st = (int(v) for v in g[f"c{case}_patch"])
    bb = StubBackbone()
    clip = Clip("stub", None, backbone=bb, tokenizer=None).cuda()
    planar = rgb.cuda()
    channel_last = rgb.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)  # [B,H,W,3] storage, [B,3,H,W] view
    for x in (planar, channel_last):
        tiles = clip.tiles_224(x, ps, st)
        assert tiles.dtype == torch.float32 and tiles.shape[1:] == (3, 224, 224)
        np.testing.assert_allclose(tiles[:, :, ::13, ::11].cpu().numpy(), g[f"c{case}_resized_sample"], rtol=0, atol=2e-6)
        np.testing.assert_allclose(tiles.double().sum(dim=(1, 2, 3)).cpu().numpy(), g[f"c{case}_resized_sum"], rtol=1e-6)
        bb.seen.clear()
        feats = clip.img_inference_tiled(x, ps, st)
        np.testing.assert_allclose(feats.cpu().numpy(), g[f"c{case}_feats"], rtol=1e-5, atol=2e-6)
    # the dtype the ViT consumes under autocast
    with torch.autocast("cuda", dtype=torch.bfloat16):
        t16 = clip.tiles_224(planar, ps, st)
    assert t16.dtype == torch.bfloat16
    ref = clip.tiles_224(planar, ps, st)
    assert torch.equal(t16, ref.to(torch.bfloat16)), "bf16 tiles are the fp32 tiles rounded once"
    with pytest.raises(AssertionError):
        clip.tiles_224(planar[:, :, :-1], ps, st)


@pytest.mark.gpu
def test_integrate_with_depth_scaled_patches_matches_the_oracle(oracle):
    """ClipFusion(scale_patches_by_depth=True).integrate (clipfusion.py:631-645): the full-resolution feature image of
    img_inference_tiled_depthscaled goes through the fused path (a 64 x 48-position map: the per-frame pipeline with its map
    image in the workspace) and equals the oracle fed with the same image."""
    from spatially_aware_ai_amd import ClipFusion
    from spatially_aware_ai_amd import synthetic as syn

    w, h = 64, 48
    grid = syn.make_grid((24, 20, 28))
    frames = syn.make_frames(77, 3, width=w, height=h, feat_dim=12, npy=1, npx=1, depth_kind="B", missing_depth_frac=0.1)
    clip = Clip("stub", None, backbone=StubBackbone(), tokenizer=None).cuda()
    fz = ClipFusion(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, True, clip, None, 16, 8, keep_xyz_world=False).cuda()
    vol = oracle.OracleVolume(grid.origin, grid.voxel_size, grid.nvox, grid.trunc, 12, 0)
    for f in frames:
        args = [f[k].cuda() for k in ("depth", "rgb", "pose", "K")]
        fz.integrate(*args)
        feat = clip.img_inference_tiled_depthscaled(args[1].permute(0, 3, 1, 2), args[0], args[3], 8).cpu()
        assert feat.shape == (1, 12, h, w)
        vol.integrate(f["depth"], f["rgb"], f["pose"], f["K"], feat)
    assert torch.equal(fz.weight.cpu(), vol.weight) and int(vol.weight.sum()) > 1000
    np.testing.assert_allclose(fz.clip_feat.cpu().numpy(), vol.clip_feat.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(fz.rgb.cpu().numpy(), vol.rgb.numpy(), rtol=1e-4, atol=1e-6)


# ------------------------------------------------------------------------------------ whole tiles against the float64 statement
# (H, W, patch, stride, out): no overlap; overlapping patches; patch 1 (all four taps are one pixel); patch 2; scale 1; downsampling;
# a second workgroup in x (out > 256); an odd small output
TILE_CASES = [(40, 56, 8, 8, 224), (40, 56, 24, 16, 224), (5, 7, 1, 2, 224), (6, 8, 2, 2, 224), (224, 224, 224, 1, 224),
              (300, 300, 300, 1, 224), (40, 56, 8, 8, 300), (40, 56, 8, 8, 37)]
_TORCH_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}  # SAF_F32, SAF_BF16, SAF_F16


@functools.lru_cache(maxsize=2)
def _tile_case(case):
    """White noise (R is large everywhere), batch 2, and the float64 statement of its tiles -- computed once per case (the
    statements of the larger cases are hundreds of MB: only the last two are kept)."""
    h, w, patch, stride, out = case
    g = torch.Generator().manual_seed(h * 1000 + patch * 10 + out)
    rgb = torch.rand(2, 3, h, w, generator=g)
    return rgb, R.tiles_f64(rgb.numpy(), patch, stride, out)


def _clip_tiles(x, patch, stride, out, dtype=torch.float32, fill=None):
    """saf_clip_tiles through the C entry (tiles_224 fixes out_size to 224), on any [B, 3, H, W] view."""
    from spatially_aware_ai_amd._lib import current_stream_ptr, lib

    bsz, _, h, w = x.shape
    tiles = bsz * (1 + (h - patch) // stride) * (1 + (w - patch) // stride)
    dst = torch.empty((tiles, 3, out, out), dtype=dtype, device=x.device)
    if fill is not None:
        dst.fill_(fill)
    mean, std = (C.c_float * 3)(*R.CLIP_MEAN), (C.c_float * 3)(*R.CLIP_STD)
    sb, sc, sy, sx = x.stride()
    rc = lib().saf_clip_tiles(x.data_ptr(), bsz, h, w, sb, sc, sy, sx, patch, stride, out, mean, std, dst.data_ptr(), _TORCH_DT[dtype],
                              current_stream_ptr())
    return rc, dst


@pytest.mark.gpu
@pytest.mark.parametrize("case", TILE_CASES, ids=str)
def test_whole_tiles_against_float64(case):
    """Every pixel of every tile, planar and channel-last, batch 2: |got - want| <= E.  fp16 and bf16 outputs are the fp32
    output rounded once.  Largest observed err / E on the MI355X per case (planar and channel-last alike), in the order of
    TILE_CASES: 0.205, 0.131, 0.153, 0.199, 0.049, 0.019, 0.189, 0.159."""
    h, w, patch, stride, out = case
    rgb, (want, rng, mag) = _tile_case(case)
    planar = rgb.cuda()
    channel_last = rgb.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
    assert channel_last.stride(1) == 1
    for name, x in (("planar", planar), ("channel-last", channel_last)):
        rc, got = _clip_tiles(x, patch, stride, out)
        assert rc == 0 and got.shape == want.shape
        ratio = R.tile_error_ratio(got.cpu().numpy(), want, rng, mag, patch)
        print(f"tiles {case} {name}: max err / E = {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)
        if name == "planar":
            ref32 = got
        else:
            assert torch.equal(got, ref32), "the layout changes addresses, not values"
    for dt in (torch.bfloat16, torch.float16):
        rc, got16 = _clip_tiles(planar, patch, stride, out, dt)
        assert rc == 0 and torch.equal(got16, ref32.to(dt)), f"{dt} tiles are the fp32 tiles rounded once"
    if out == 224:  # the route integrate() takes
        clip = Clip("stub", None, backbone=StubBackbone(), tokenizer=None).cuda()
        assert torch.equal(clip.tiles_224(planar, patch, stride), ref32)
        assert torch.equal(clip.tiles_224(channel_last, patch, stride, dtype=torch.float16), ref32.half())
    if patch == out:  # scale 1: w1 = h1 = 0 -- the normalised input, exactly
        m, s = (torch.tensor(v).view(1, 3, 1, 1) for v in (R.CLIP_MEAN, R.CLIP_STD))
        assert torch.equal(ref32.cpu(), (rgb - m) / s)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(40, 56, 24, 16, 224), (40, 56, 8, 8, 37), (6, 8, 2, 2, 224)], ids=str)
def test_tiles_of_a_centre_crop_view(case):
    """A centre crop of a larger frame: stride_y != W * stride_x and a storage offset, planar and channel-last.  The tiles are
    those of the crop's own copy, bit for bit, and the destination beyond them is left alone."""
    h, w, patch, stride, out = case
    rgb, (want, rng, mag) = _tile_case(case)
    big = torch.rand(2, 3, h + 7, w + 10, generator=torch.Generator().manual_seed(5))
    big[:, :, 3:3 + h, 6:6 + w] = rgb
    for name, frame in (("planar", big.cuda()), ("channel-last", big.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2))):
        x = frame[:, :, 3:3 + h, 6:6 + w]
        assert x.storage_offset() != 0 and x.stride(2) != w * x.stride(3)
        rc, got = _clip_tiles(x, patch, stride, out)
        assert rc == 0
        ratio = R.tile_error_ratio(got.cpu().numpy(), want, rng, mag, patch)
        assert ratio <= 1.0, (name, ratio)
        rc, plain = _clip_tiles(rgb.cuda(), patch, stride, out)
        assert rc == 0 and torch.equal(got, plain)


@pytest.mark.gpu
def test_clip_tiles_refusals():
    """patch > H, (W - patch) % stride != 0 and more than 65535 tiles are refused, and nothing is written."""
    from spatially_aware_ai_amd import _abi
    from spatially_aware_ai_amd._lib import current_stream_ptr, lib

    x = torch.rand(1, 3, 40, 56, device="cuda")
    mean, std = (C.c_float * 3)(*R.CLIP_MEAN), (C.c_float * 3)(*R.CLIP_STD)
    dst = torch.full((66000 * 3,), 7.0, device="cuda")

    def call(t, patch, stride, out=1):
        sb, sc, sy, sx = t.stride()
        return lib().saf_clip_tiles(t.data_ptr(), t.shape[0], t.shape[2], t.shape[3], sb, sc, sy, sx, patch, stride, out, mean, std,
                                    dst.data_ptr(), _abi.SAF_F32, current_stream_ptr())

    assert call(x, 41, 1) == _abi.SAF_E_INVALID                     # patch > H
    assert call(x, 8, 32) == _abi.SAF_E_INVALID                     # (H - patch) % stride == 0, (W - patch) % stride != 0
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()), "a refused call wrote nothing"
    assert call(x[:, :, :, :40], 8, 32) == _abi.SAF_OK              # ... and with W = 40 it is taken: 2 x 2 tiles of one pixel
    many = torch.rand(1, 3, 256, 257, device="cuda")
    assert call(many, 1, 1) == _abi.SAF_E_UNSUPPORTED               # 256 * 257 = 65792 tiles
    assert call(many[:, :, :255], 1, 1) == _abi.SAF_OK              # 255 * 257 = 65535: the most one call takes
    torch.cuda.synchronize()
    assert bool((dst[65535 * 3:] == 7.0).all()) and bool((dst[:65535 * 3] != 7.0).all())
    m, s = (torch.tensor(v).view(3, 1, 1) for v in (R.CLIP_MEAN, R.CLIP_STD))
    assert torch.equal(dst[:65535 * 3].view(255, 257, 3).cpu(), ((many[0, :, :255].cpu() - m) / s).permute(1, 2, 0))
