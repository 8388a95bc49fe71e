"""CPU: which path a fusion call takes and what workspace it is told to bring, replayed from tests/golden/fuse_route_table.json
(recorded by tools/gen_fuse_route_table.py): saf_fuse_workspace_bytes, _for and _for_frames, saf_fuse_path and
saf_fuse_session_ok over feature widths, dtypes, grids, frame lists, workspace sizes at and one byte below every sizing answer,
and the SAF_* environments that steer the route.  The five entries make no HIP call and follow no device pointer."""
import importlib.util
import json
import os

import pytest

from spatially_aware_ai_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fuse_route_table.json")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_fuse_route_table", os.path.join(ROOT, "tools", "gen_fuse_route_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("block", ["widths", "frames", "modes"])
def test_route_table_replays(gen, table, block):
    assert (table["frame_height"], table["frame_width"]) == (gen.H, gen.W)
    b = table["blocks"][block]
    cases, rows = list(gen.cases(b["axes"])), gen.decode(b)
    assert len(cases) == len(rows) and len(cases) > 0
    lib = _lib.lib()
    wrong = [(c, got, want) for c, want in zip(cases, rows) for got in [gen.evaluate(lib, c)] if got != want]
    assert not wrong, f"{len(wrong)} of {len(cases)} cases differ; first: {wrong[0]}"


def test_route_table_covers_what_it_should(gen, table):
    """The recorded table is the one the generator describes, and it holds every kind of answer."""
    assert {k: v["axes"] for k, v in table["blocks"].items()} == gen.BLOCKS
    rows = [r for b in table["blocks"].values() for r in gen.decode(b)]
    assert len(rows) == 5008
    assert {ch for r in rows for ch in r[3]} == {"0", "1"} and {ch for r in rows for ch in r[4]} == {"0", "1"}
    assert any(r[0] != r[1] for r in rows) and any(r[1] != r[2] for r in rows)
    # a workspace one byte short of a sizing answer changes the route somewhere
    assert any(r[3][i] != r[3][i + 1] for r in rows for i in (0, 2, 4))
