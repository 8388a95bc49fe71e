#!/usr/bin/env python3
"""Generates tests/golden/object_bookkeeping.json: the reference's own ``merge_objects`` and ``mark_object_of_interest``
(handy_utils.py:501-582) run on the first-scan ``scene_knowledge`` that tests/golden/label_components.npz pins (case 0:
its label grid, object ids, indices and classes as ``flood_fill_3d`` left them), inputs and resulting dictionaries stored for
tests/test_objects_host.py.

Steps, each on the result of the one before: a two-object merge, a single-object rename, a rename to a label that already
carries ``:n``, and ``mark_object_of_interest`` (one id of them unknown).  The output is data only.  The script does nothing
when the reference is absent.
Usage:  python tools/gen_golden_objects.py [--out tests/golden]
"""
import argparse
import contextlib
import copy
import io
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


def first_scan_knowledge(golden_dir, case=0):
    """The ``scene_knowledge`` of a first scan (handy_utils.py:430-452) rebuilt from the pinned arrays; voxels in raster order."""
    g = np.load(os.path.join(golden_dir, "label_components.npz"))
    ids = [str(s) for s in g[f"c{case}_ids"]]
    index = g[f"c{case}_object_index"].tolist()
    class_id = g[f"c{case}_class_id"].tolist()
    names = [str(s) for s in g[f"c{case}_class_names"]]
    grid = g[f"c{case}_voxel_obj_ids"]
    unique_objects, object_counts = {}, {}
    for oid, oi, ci in zip(ids, index, class_id):
        label = names[ci]
        object_counts[label] = object_counts.get(label, 0) + 1
        unique_objects[oid] = {
            "class_id": int(ci), "class_label": label, "voxels": [list(map(int, v)) for v in np.argwhere(grid == oi)],
            "object_index": int(oi), "gt_label": oid, "user_modified": False, "merged": False, "removed": False, "color": None,
        }
    return {"unique_objects": unique_objects, "object_counts": object_counts, "unchanged_objects": {}, "new_objects": {},
            "missing_objects": {}}


def steps_for(knowledge):
    ids = list(knowledge["unique_objects"])
    return [
        {"op": "merge_objects", "merge_list": [ids[1], ids[3]], "new_label": "shelf"},
        {"op": "merge_objects", "merge_list": [ids[0]], "new_label": "my mug"},
        {"op": "merge_objects", "merge_list": [ids[2]], "new_label": ids[4]},  # a label that already carries ":n"
        {"op": "merge_objects", "merge_list": [], "new_label": "nothing"},
        {"op": "mark_object_of_interest", "object_list": [ids[5], "no such object:1", ids[6]]},
        {"op": "mark_object_of_interest", "object_list": []},
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    if not os.path.isdir(REF):
        print("no reference checkout: nothing generated")
        return
    sys.path.insert(0, REPO)
    from oracle.gen_golden import import_reference

    import_reference()
    import handy_utils as hu

    class _Model:
        def __init__(self):
            self.labels = ["null"]
            self.model_trained = False

    knowledge = first_scan_knowledge(args.out)
    model = _Model()
    record = {"labels": list(model.labels), "scene_knowledge": copy.deepcopy(knowledge), "steps": []}
    for step in steps_for(knowledge):
        with contextlib.redirect_stdout(io.StringIO()):  # the reference prints
            if step["op"] == "merge_objects":
                ret = hu.merge_objects(knowledge, None, model, list(step["merge_list"]), step["new_label"])
                new_id, knowledge = ret if isinstance(ret, tuple) else (None, ret)
            else:
                new_id, knowledge = None, hu.mark_object_of_interest(knowledge, model, list(step["object_list"]))
        record["steps"].append(dict(step, new_id=new_id, labels=list(model.labels), scene_knowledge=copy.deepcopy(knowledge)))
    path = os.path.join(args.out, "object_bookkeeping.json")
    with open(path, "w") as f:
        json.dump(record, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes;", [s["new_id"] for s in record["steps"]])


if __name__ == "__main__":
    main()
