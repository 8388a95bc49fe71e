"""GPU: every fusion form on feature maps unlike N(0,1), bounded per CHANNEL (tests/feature_family_reference.py).

Forms: the per-frame pipeline (calls of 7 frames), SAF_WIN_FORM=rows, sums, bricks at D = 256, and the default form at D = 320
(the brick form: no row kernel takes that width); f32, bf16 and fp16 volumes wherever tests/golden/fuse_route_table.json sends the
combination to the windowed path -- it sends 16-bit volumes of D = 256 to the brick form only, so their rows and sums forms
(the 16-bit map images) run at D = 512 -- (the table's 16-bit axis is bf16: an fp16 volume takes the same row kernels and never
the brick form, which tests/test_fp16_volume_gpu.py pins); SAF_SUM on f32; one ClipSeemFusion case per form; and 140 frames -- the scene's
40 over and over with fresh maps -- for the second window's blend (w0 old + sum) / (w0 + k).

Per (form, family), one test:
  a. weight, tsdf_weight, tsdf, rgb, the label histogram and stats() equal the per-frame pipeline's AND the N(0,1) run's (the
     families touch only the maps);
  b. f32: |got - float64 mean| <= c_form(k) 2^-24 T[v, c] (+ the brick form's fixed-point term), element by element, c_form
     derived in ``feature_family_reference.roundings``; SAF_SUM: the same bar, times k, on the sums;
  c. bf16 / fp16: the same shape with the narrowings counted per form (``roundings16``);
  d. up40 / dn40 / neg: the N(0,1) result times 2^+-40 / negated, BIT FOR BIT (up to the sign of a zero);
  e. a second run returns equal bytes.
Every touched row and every channel is compared; the untouched rows must be zero bits.

Measured on an MI355X, largest used fraction of the bound (n01 / unit / outlier / spatial; `-s` prints each):
  f32    frame 0.08 / 0.10 / 0.08 / 0.08 (rows: the same bits)   sums 0.18 / 0.23 / 0.18 / 0.18   bricks 0.27 / 0.34 / 1.00 / 0.99
         default at D = 320: 0.29 / 0.33 / 1.00 / 0.99           SAF_SUM: 0.05-0.06, 0.18-0.23, and the brick form's as above
  bf16   frame 0.93-0.97 (rows at D = 512: the same bits)         sums 0.90 / 0.82 / 0.90 / 0.90   bricks 0.94 / 0.93 / 0.88 / 0.92
  fp16   frame, rows 0.95 / 0.94 / 0.95 / 0.95                    sums 0.81 / 0.84 / 0.81 / 0.81
  140 frames, f32: rows 0.07 / 0.14 / 0.07 / 0.07, sums 0.07 / 0.10 / 0.07 / 0.07, bricks 0.12 / 0.15 / 0.90 / 0.91.
(A row hit once holds one rounded sample: the 16-bit bounds and the brick form's half unit are met, not merely approached.)
An ordinary channel beside the x 4096 channel in the brick form at D = 256 (one slab): the bound is 3.4e-4 of its own T (the
fixed-point unit is the slab's); measured 3.3e-4.  At D = 320 (slabs of 64) channels 128..191 share no slab with a loud channel:
their bound is 1.0e-5 of T, measured 2.2e-7.

Found by d.: the brick form rounded its fixed-point samples with floor(x + 0.5); on negated maps 26 % of the values (f32) were not
the negated N(0,1) values.  saf_brick.hip now rounds ties to even."""
import importlib.util
import json
import math
import os
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from spatially_aware_ai_amd import _abi

import feature_family_reference as ffr
from test_brick_form import EXACT, _build, _fuse

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
MEAN, SUM = _abi.SAF_RUNNING_MEAN, _abi.SAF_SUM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_ENV = {"frame": None, "rows": "rows", "sums": "sums", "bricks": "bricks", "default": None}


@dataclass(frozen=True)
class Config:
    form: str       # frame | rows | sums | bricks | default
    dim: int
    dtype: torch.dtype
    accum: int = MEAN
    seem: bool = False
    n_frames: int = ffr.N_FRAMES

    @property
    def arithmetic(self):
        """Whose rounding count applies: the default form at a width no row kernel takes is the brick form."""
        return "bricks" if self.form == "default" else self.form

    @property
    def windows(self):
        return 1 if self.form == "frame" else math.ceil(self.n_frames / ffr.SUM_WINDOW)

    @property
    def group(self):
        """What the per-frame baseline depends on."""
        return (self.dim, self.dtype, self.accum, self.seem, self.n_frames)

    def __str__(self):
        return "-".join([self.form, f"D{self.dim}", str(self.dtype).split(".")[1]] + (["sum"] if self.accum == SUM else []) +
                        (["seem"] if self.seem else []) + ([f"{self.n_frames}f"] if self.n_frames != ffr.N_FRAMES else []))


def _route_table_windowed():
    """{(feat_dim, bf16, SAF_WIN_FORM or None)}: the combinations the recorded route table sends a 16-frame call to the windowed
    path (block "widths", the 61 x 60 x 59 grid, a workspace of the size the library asks for)."""
    spec = importlib.util.spec_from_file_location("gen_fuse_route_table", os.path.join(ROOT, "tools", "gen_fuse_route_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    block = json.load(open(os.path.join(ROOT, "tests", "golden", "fuse_route_table.json")))["blocks"]["widths"]
    out = set()
    for case, row in zip(gen.cases(block["axes"]), gen.decode(block)):
        env = case["env"]
        if case["grid"] == [61, 60, 59] and set(env) <= {"SAF_WIN_FORM"} and row[3][0] == "1":
            out.add((case["feat_dim"], case["bf16"], env.get("SAF_WIN_FORM")))
    return out


def _configs():
    table = _route_table_windowed()
    out = []

    def add(form, dim, dtype, **kw):
        # (the table's 16-bit axis is bf16; an fp16 volume takes the same row kernels -- row_kernel_takes knows "16-bit rows" only --
        #  and never the brick form: tests/test_fp16_volume_gpu.py)
        if form != "frame" and (dim, int(dtype != F32), FORM_ENV[form]) not in table:
            return  # the route table sends this combination to the per-frame pipeline (16-bit rows / sums at D = 256)
        out.append(Config(form, dim, dtype, **kw))

    for dtype in (F32, BF16):
        for form in ("frame", "rows", "sums", "bricks"):
            add(form, 256, dtype, seem=dtype == F32)  # f32: one ClipSeemFusion case per form
        add("frame", 320, dtype, seem=dtype == F32)
        add("default", 320, dtype, seem=dtype == F32)
    for dtype in (BF16, F16):  # the 16-bit row kernels start at D = 512
        for form in ("frame", "rows", "sums"):
            add(form, 512, dtype)
    for form in ("frame", "rows", "sums", "bricks"):
        add(form, 256, F32, accum=SUM)
    for form in ("frame", "rows", "sums", "bricks"):
        add(form, 256, F32, n_frames=140)
    return out


CONFIGS = _configs()
CASES = [(c, fam) for c in CONFIGS for fam in ffr.FAMILIES if not (c.dtype == F16 and fam in ("up40", "dn40"))]  # 2^40 is no half


def test_the_route_table_allows_every_form_of_the_issue():
    """f32 takes all five forms at D = 256 / 320; bf16 the brick form there and the row forms at D = 512, fp16 the row forms at
    D = 512; SAF_SUM and the 140 frames four forms each."""
    names = [str(c) for c in CONFIGS]
    assert len(CONFIGS) == 6 + (4 + 3) + 3 + 4 + 4, names
    assert "rows-D256-bfloat16" not in names and "sums-D512-bfloat16" in names and "sums-D512-float16" in names


# ---- running a configuration ------------------------------------------------------------------------------------------------
_scenes, _refs, _baseline, _plain = {}, {}, {}, {}


def _frames(cfg, family):
    key = (cfg.dim, cfg.n_frames)
    if key not in _scenes:
        _scenes.clear()
        _scenes[key] = ffr.scene(cfg.dim, cfg.n_frames)
    return ffr.apply_family(_scenes[key], family)


def _reference(oracle, cfg, family):
    key = (cfg.dim, cfg.n_frames, family)
    if key not in _refs:
        for old in [k for k in _refs if k[:2] != key[:2]]:
            del _refs[old]
        oracle.set_threads(8)
        try:
            _refs[key] = ffr.float64_mean(oracle, ffr.grid(), _frames(cfg, family), cfg.dim, False)
        finally:
            oracle.set_threads(1)
    return _refs[key]


def _run(cfg, frames, monkeypatch):
    """Fuse and bring back everything the test compares: the exact buffers, stats(), and the feature rows in the volume's type."""
    if FORM_ENV[cfg.form] is None:
        monkeypatch.delenv("SAF_WIN_FORM", raising=False)
    else:
        monkeypatch.setenv("SAF_WIN_FORM", FORM_ENV[cfg.form])
    grid = ffr.grid()
    if cfg.form == "frame":  # calls of 7 frames take the per-frame pipeline (bit-identical to frame after frame)
        fz = _fuse(_build(grid, cfg.dim, cfg.seem, cfg.accum, cfg.dtype, defer=False), frames, cfg.seem, per_call=7)
    else:
        fz = _fuse(_build(grid, cfg.dim, cfg.seem, cfg.accum, cfg.dtype), frames, cfg.seem)
    st = fz.stats()
    st.pop("window_form")  # (derived from the environment at the time of the call, not from the run)
    out = {name: getattr(fz, name).cpu() for name in EXACT + (("labels_one_hot",) if cfg.seem else ())}
    out["clip_feat"] = fz.clip_feat.cpu()
    out["window_rows"] = st.pop("window_rows")
    st.pop("window_tsdf_voxels")
    out["cull_pairs"] = st.pop("cull")["pairs"]
    out["stats"] = st
    return out


def _baseline_of(cfg, family, monkeypatch):
    """The per-frame pipeline's run of the configuration's volume (shared by the forms of one group)."""
    key = cfg.group + (family,)
    if key not in _baseline:
        for old in [k for k in _baseline if k[:-1] != cfg.group]:
            del _baseline[old]
        base_cfg = Config("frame", cfg.dim, cfg.dtype, cfg.accum, cfg.seem, cfg.n_frames)
        _baseline[key] = _run(base_cfg, _frames(cfg, family), monkeypatch)
    return _baseline[key]


def _plain_of(cfg, monkeypatch):
    """The configuration's run on the N(0,1) maps: what the exact buffers of every family, and the scaled families' bits, must equal."""
    if cfg not in _plain:
        _plain.clear()
        _plain[cfg] = _baseline_of(cfg, "n01", monkeypatch) if cfg.form == "frame" else _run(cfg, _frames(cfg, "n01"), monkeypatch)
    return _plain[cfg]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _scene_conditions(weight, n_frames):
    """feature_family_reference.scene_conditions on the device's own weight; 140 frames are 3.5 passes over the same cameras: a row
    of one hit per pass has 3 or 4, one of 33 or more per pass 99 or more."""
    w = weight.numpy().reshape(-1)
    if n_frames == ffr.N_FRAMES:
        return ffr.scene_conditions(w)
    passes = n_frames // ffr.N_FRAMES
    got = int((w > 0).sum()), int((w >= 33 * passes).sum()), int(((w == passes) | (w == passes + 1)).sum())
    assert got[0] >= 5000 and got[1] >= 1000 and got[2] >= 1000 and int(w.max()) > ffr.SUM_WINDOW, got
    return got


# ---- the test ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,family", CASES, ids=[f"{c}-{fam}" for c, fam in CASES])
def test_family(oracle, monkeypatch, cfg, family):
    frames = _frames(cfg, family)
    base = _baseline_of(cfg, family, monkeypatch)
    got = base if cfg.form == "frame" else _run(cfg, frames, monkeypatch)
    again = _run(cfg, frames, monkeypatch)
    if family == "n01" and cfg not in _plain:
        _plain.clear()
        _plain[cfg] = got
    plain = _plain_of(cfg, monkeypatch)
    what = f"{cfg}, {family}"

    # guards: the form ran, on the rows the scene was built for
    assert base["window_rows"] == 0 and base["cull_pairs"] == 0, "the baseline did not take the per-frame pipeline"
    if cfg.form != "frame":
        assert got["window_rows"] > 0 and got["cull_pairs"] > 0, f"{what}: the windowed path did not run"
    _scene_conditions(got["weight"], cfg.n_frames)

    # a. exact things stay exact, on every family
    for other, whose in ((base, "the per-frame pipeline's"), (plain, "the N(0,1) run's")):
        assert got["stats"] == other["stats"], (what, whose, got["stats"], other["stats"])
        for name in EXACT + (("labels_one_hot",) if cfg.seem else ()):
            assert torch.equal(got[name], other[name]), f"{what}: {name} differs from {whose}"

    # e. run to run
    assert torch.equal(_bits(again["clip_feat"]), _bits(got["clip_feat"])), f"{what}: two runs differ"
    for name in EXACT:
        assert torch.equal(again[name], got[name]), f"{what}: {name} differs between two runs"

    touched = got["weight"].reshape(-1) > 0
    feat = got["clip_feat"]
    assert feat.dtype == cfg.dtype
    assert not bool(_bits(feat[~touched]).any()), f"{what}: an untouched row is not zero bits"

    if family in ffr.EXACT_IMAGE:
        # d. nothing in the documented arithmetic knows the absolute scale or the sign: bit for bit (a power of two is exact in
        #    every one of the three types; equal values of finite numbers are equal bits, but for the sign of a zero)
        want = (plain["clip_feat"].double() * ffr.EXACT_IMAGE[family]).to(cfg.dtype)
        assert torch.equal(want.double(), plain["clip_feat"].double() * ffr.EXACT_IMAGE[family]), "the image is not exact in this type"
        assert bool(torch.isfinite(feat[touched].float()).all()), f"{what}: non-finite values"
        differ = feat != want
        n_bad = int(differ.sum())
        if n_bad:
            rel = ((feat.double() - want.double()).abs() / want.double().abs().clamp_min(1e-300))[differ]
            assert False, f"{what}: {n_bad} of {int(touched.sum()) * cfg.dim} values are not the N(0,1) run's x {ffr.EXACT_IMAGE[family]:g}; " \
                          f"largest relative difference {float(rel.max()):.3g}"
        nz = want != 0
        assert torch.equal(_bits(feat)[nz], _bits(want)[nz])
        return

    # b. / c. per channel against float64
    ref = _reference(oracle, cfg, family)
    assert np.array_equal(ref.k, got["weight"].numpy().reshape(-1)), f"{what}: weight is not the count of the frames that hit"
    fixed = None
    if cfg.arithmetic == "bricks":
        k_max = min(int(ref.k.max()), ffr.SUM_WINDOW)
        fixed = ffr.brick_fixed_point(frames, cfg.dim, k_max)
    bound = ffr.per_channel_bound(cfg.arithmetic, cfg.dtype, ref, accum_sum=cfg.accum == SUM, windows=cfg.windows, fixed_point=fixed)
    rows = torch.from_numpy(ref.rows)
    ffr.assert_per_channel(feat[rows].double().numpy(), ref.target(cfg.accum == SUM), bound, what)
    if family == "outlier" and cfg.arithmetic == "bricks" and cfg.accum == MEAN:
        # how coarse an ordinary channel may get beside a loud one: the bound relative to the channel's own T, for the channels
        # of the x 4096 channel's slab and for channels 128..191 (a slab of their own at D = 320, not at D = 256)
        slab = ffr.brick_slab_channels(cfg.dim)
        loud = set(ffr.outlier_channels(cfg.dim))
        beside = [c for c in range(200 // slab * slab, 200 // slab * slab + slab) if c not in loud]
        rel = bound / ref.T
        err = np.abs(feat[rows].double().numpy() - ref.mean) / ref.T
        print(f"{what}: an ordinary channel of the x 4096 channel's slab may be off by {rel[:, beside].max():.3g} of its own T "
              f"(measured {err[:, beside].max():.3g}); channels 128..191: {rel[:, 128:192].max():.3g} (measured {err[:, 128:192].max():.3g})")
