#!/usr/bin/env python3
"""Writes tests/golden/fuse_route_table.json: what the five host-only entry points that decide a fusion call's route return
over a table of volumes, frame lists, workspace sizes and SAF_* environments --

    saf_fuse_workspace_bytes, saf_fuse_workspace_bytes_for, saf_fuse_workspace_bytes_for_frames,
    saf_fuse_path, saf_fuse_session_ok.

None of them makes a HIP call or follows a device pointer (they read struct fields and the environment), so the table is
recorded and replayed on a machine without a GPU, with placeholder addresses.  tests/test_fuse_route_host.py replays it against
the built library and asserts every value: a refactor of the routing rules must leave the file as it is, and a change of
behaviour shows up as a diff of it.

The file holds, per block, the axes (lists of values; a case is one element of their product, in the order the axes are
listed, last axis fastest), the distinct triples of sizing answers ("sizes": [bytes, bytes_for, bytes_for_frames]) and the
cases' results in product order as run-length tokens "<n>*<i>.<path>.<session>": n consecutive cases (1 when "<n>*" is absent)
whose sizes are triple i and whose saf_fuse_path / saf_fuse_session_ok answers are `path` / `session` -- two hex digits, one bit
per workspace size (the three sizing answers and one byte less than each, in the order a, a - 1, b, b - 1, c, c - 1; the first
is the highest of the six bits), 1 where the entry returned 1.  (Both entries return -1 only for an invalid volume or an empty
frame list; the table has neither, and encode() refuses one.)  decode() gives back one row per case:
[bytes, bytes_for, bytes_for_frames, path, session] with path and session as strings of six "0" / "1".

Usage:  python tools/gen_fuse_route_table.py [--out tests/golden/fuse_route_table.json]
(SAF_LIB_PATH selects the build to record from.)
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from spatially_aware_ai_amd import _abi  # noqa: E402

WIDTHS = [32, 48, 64, 128, 192, 256, 320, 512, 768, 1024, 1280, 2048, 8192, 8256]
# (the last grid has 1024 bricks of 4 voxels along x: one more than the brick form's 10-bit brick coordinates hold)
GRIDS = [[8, 8, 8], [61, 60, 59], [256, 256, 256], [4096, 4, 4]]
ENVS = [{}, {"SAF_WIN_FORM": "rows"}, {"SAF_WIN_FORM": "sums"}, {"SAF_WIN_FORM": "bricks"}, {"SAF_WINDOW": "0"},
        {"SAF_WINDOW_BF16": "0"}, {"SAF_WIN_FRAMES": "64"}, {"SAF_WIN_OVERLAP": "0"}, {"SAF_CLS_TILED": "0"}, {"SAF_WIN_MAPS16": "0"}]
WIN_MIN_FRAMES = 16  # kWinMinFrames (saf_window.hip)
FRAME_COUNTS = [1, WIN_MIN_FRAMES - 1, WIN_MIN_FRAMES, 128, 129]
MAPS = [[30, 40], [30, 252], [30, 253]]  # [npy, npx]: npx + 3 = 43, 255 and 256 (a hit's map cell travels as two bytes)
# a frame list: every frame alike / the last frame of another shape / label_map on every other frame only
LISTS = ["uniform", "one_other_shape", "labels_on_some"]
H, W = 480, 640

# block -> axes, in product order.  Every width, dtype, grid and environment meet in "widths"; the frame list's axes meet four
# widths (brick form by default, row kernel for f32 only, row kernel for both, brick form beyond the row kernel) in every
# environment; the accumulation mode and label counting (they size the workspace and pick kernels, not routes) in "modes".
BLOCKS = {
    "widths": {"feat_dim": WIDTHS, "bf16": [0, 1], "grid": GRIDS, "env": ENVS, "accum": [0], "n_classes": [0],
               "n_frames": [WIN_MIN_FRAMES], "map": MAPS[:1], "frames": LISTS[:1]},
    "frames": {"feat_dim": [64, 256, 512, 1280], "bf16": [0, 1], "grid": GRIDS[1:2], "env": ENVS, "accum": [0], "n_classes": [0],
               "n_frames": FRAME_COUNTS, "map": MAPS, "frames": LISTS},
    "modes": {"feat_dim": [64, 512, 768], "bf16": [0, 1], "grid": [GRIDS[0], GRIDS[2]], "env": [ENVS[0], ENVS[2], ENVS[8]],
              "accum": [0, 1], "n_classes": [0, 7], "n_frames": [WIN_MIN_FRAMES], "map": MAPS[:1], "frames": ["uniform", "labels_on_all"]},
}

ADDR = 0x7F0000000000  # a non-null, 256-byte aligned placeholder: the entries never follow it


def make_volume(case):
    v = _abi.SafVolume()
    v.nx, v.ny, v.nz = case["grid"]
    v.feat_dim = case["feat_dim"]
    v.n_classes = case["n_classes"]
    v.feat_dtype = _abi.SAF_BF16 if case["bf16"] else _abi.SAF_F32
    v.accum_mode = case["accum"]
    v.trunc = 0.1
    for name in ("axis_x", "axis_y", "axis_z", "tsdf", "tsdf_weight", "weight", "rgb", "clip_feat"):
        setattr(v, name, ADDR)
    v.labels_one_hot = ADDR if case["n_classes"] else None
    return v


def make_frames(case):
    n = case["n_frames"]
    frames = (_abi.SafFrame * n)()
    for i, f in enumerate(frames):
        f.height, f.width = H, W
        f.depth = f.rgb = f.pose = f.K = f.feat_map = ADDR
        f.npy, f.npx = case["map"]
        f.rgb_bilinear = 0
        kind = case["frames"]
        f.label_map = ADDR if kind == "labels_on_all" or (kind == "labels_on_some" and i % 2 == 1) else None
        if kind == "one_other_shape" and i == n - 1 and n > 1:
            f.height, f.width = H // 2, W // 2
    return frames


def set_env(env):
    for e in ENVS:
        for k in e:
            os.environ.pop(k, None)
    os.environ.update(env)  # (os.environ writes through to the C environment that the library reads per call)


def evaluate(lib, case):
    """One row of the table: the five entries' answers for `case` (a dict with one value per axis)."""
    set_env(case["env"])
    try:
        vol, frames = make_volume(case), make_frames(case)
        n_vox = case["grid"][0] * case["grid"][1] * case["grid"][2]
        npy, npx = case["map"]
        sizes = [int(lib.saf_fuse_workspace_bytes(n_vox, case["feat_dim"], npy, npx)),
                 int(lib.saf_fuse_workspace_bytes_for(C.byref(vol), npy, npx)),
                 int(lib.saf_fuse_workspace_bytes_for_frames(C.byref(vol), npy, npx, H, W))]
        path = session = ""
        for b in sizes:
            for ws in (b, max(b - 1, 0)):
                path += "-01"[lib.saf_fuse_path(C.byref(vol), frames, case["n_frames"], ws) + 1]
                session += "-01"[lib.saf_fuse_session_ok(C.byref(vol), frames, case["n_frames"], ws) + 1]
        return sizes + [path, session]
    finally:
        set_env({})


def encode(rows, per_line=16):
    """Rows of evaluate() as {"sizes": distinct triples, "runs": lines of run-length tokens} (the module's docstring)."""
    sizes, tokens = [], []
    for r in rows:
        assert set(r[3] + r[4]) <= {"0", "1"}, r
        if r[:3] not in sizes:
            sizes.append(r[:3])
        tok = "%d.%02x.%02x" % (sizes.index(r[:3]), int(r[3], 2), int(r[4], 2))
        if tokens and tokens[-1][1] == tok:
            tokens[-1][0] += 1
        else:
            tokens.append([1, tok])
    words = [("%d*%s" % (n, t)) if n > 1 else t for n, t in tokens]
    return {"sizes": sizes, "runs": [" ".join(words[i:i + per_line]) for i in range(0, len(words), per_line)]}


def decode(block):
    rows = []
    for word in " ".join(block["runs"]).split():
        n, _, tok = word.rpartition("*")
        i, path, session = tok.split(".")
        rows += [block["sizes"][int(i)] + [format(int(path, 16), "06b"), format(int(session, 16), "06b")]] * int(n or 1)
    return rows


def write(path, blocks):
    lines = lambda items: ",\n".join("   " + json.dumps(x) for x in items)
    triples = lambda t: ",\n".join("   " + json.dumps(t[i:i + 4])[1:-1] for i in range(0, len(t), 4))
    with open(path, "w") as f:
        f.write('{"frame_height": %d, "frame_width": %d, "blocks": {\n' % (H, W))
        for bi, (name, b) in enumerate(blocks.items()):
            f.write(' %s: {"axes": %s,\n  "sizes": [\n%s\n  ],\n  "runs": [\n%s\n  ]}%s\n'
                    % (json.dumps(name), json.dumps(b["axes"]), triples(b["sizes"]), lines(b["runs"]), "," if bi + 1 < len(blocks) else ""))
        f.write("}}\n")


def cases(axes):
    names = list(axes)
    for values in itertools.product(*(axes[k] for k in names)):
        yield dict(zip(names, values))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "fuse_route_table.json"))
    args = ap.parse_args()
    from spatially_aware_ai_amd import _lib

    lib = _lib.lib()
    blocks = {name: dict(axes=axes, **encode([evaluate(lib, c) for c in cases(axes)])) for name, axes in BLOCKS.items()}
    write(args.out, blocks)
    print(args.out, {name: len(decode(b)) for name, b in blocks.items()})


if __name__ == "__main__":
    main()
