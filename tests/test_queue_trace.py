"""GPU: the schedule of the queue behind integrate() -- which library call follows which, with how many frames, about which
ring slots, on which stream -- replayed from tests/golden/queue_trace.json (recorded by tools/gen_queue_trace.py, whose docstring
describes the tokens).  The device paths are bit-identical by design, so the parity tests cannot notice a flush that quietly
takes another route; this does.  The host decisions depend on counts and shapes alone, so the trace is deterministic."""
import importlib.util
import json
import os
import re

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "queue_trace.json")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_queue_trace", os.path.join(ROOT, "tools", "gen_queue_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def _names():
    return list(json.load(open(GOLDEN))["scenarios"])


@pytest.mark.parametrize("name", _names())
def test_queue_trace_replays(gen, golden, name):
    want = golden["scenarios"][name]
    got = gen.record(name)
    first = next((i for i, (a, b) in enumerate(zip(got["trace"], want["trace"])) if a != b), min(len(got["trace"]), len(want["trace"])))
    assert got["trace"] == want["trace"], (f"{name}: the trace differs from token {first} on: got {got['trace'][first:first + 4]}, "
                                           f"recorded {want['trace'][first:first + 4]}")
    # one more witness of the end state
    assert (got["pending"], got["frames"]) == (want["pending"], want["frames"])


def test_queue_trace_covers_what_it_should(gen, golden):
    """The recorded file is the one the generator describes and it is not vacuous: every recorded entry occurs, and so do a push
    of fewer frames than were pending (the `keep` form), the ring's wrap and a borrowed descriptor.

    The wrap: a push or a saf_fuse_session_ok call is recorded at every 32nd slot, so no single run of saf_stage_frame calls
    spans slots 511 and 0; what is asserted is a stage token that ends at slot 511 with the next stage token of its scenario
    starting at slot 0."""
    assert golden["ring_slots"] == gen.RING_SLOTS and list(golden["scenarios"]) == list(gen.SCENARIOS)
    traces = {k: v["trace"] for k, v in golden["scenarios"].items()}
    words = {t.split()[0].split("*")[0] for tr in traces.values() for t in tr}
    assert words == {"stage", "create", "ok", "prepare", "push", "finish", "abandon", "destroy", "path", "fuse", "recycled", "clear"}
    keep_form = wrap = borrowed = False
    for tr in traces.values():
        last_staged = None  # the newest staged slot
        for t in tr:
            m = re.match(r"stage\*(\d+)@(\d+)-(\d+) ", t)
            if m:
                wrap |= last_staged == gen.RING_SLOTS - 1 and int(m.group(2)) == 0
                last_staged = int(m.group(3))
            m = re.match(r"push (\d+)@(\d+):(\w) ", t)
            if m:
                n, slot = int(m.group(1)), int(m.group(2))
                keep_form |= last_staged is not None and (slot + n - 1) % gen.RING_SLOTS != last_staged
                borrowed |= m.group(3) == "c"
    assert keep_form, "no push of fewer frames than were staged"
    assert wrap, "the ring never wraps"
    assert borrowed, "no pushed descriptor points at a caller's images"
    assert os.path.getsize(GOLDEN) < 200 * 1024
