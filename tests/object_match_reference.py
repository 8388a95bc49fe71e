"""NumPy statements of saf_object_overlap (include/saf.h) and of ``objects.assign_identities`` that the tests hold the product to.
``overlap_counts`` slices the overlap box out of both grids and counts with ``np.add.at``; ``assign`` is written with explicit loops
over sorted candidate lists, independently of the product's array code."""
import numpy as np


def overlap_box(nvox_a, nvox_b, off):
    """Per axis the range [lo, hi) of b's indices whose a index (+ off) lies inside a; None where the boxes share no voxel."""
    box = []
    for k in range(3):
        lo, hi = max(0, -int(off[k])), min(int(nvox_b[k]), int(nvox_a[k]) - int(off[k]))
        if hi <= lo:
            return None
        box.append((lo, hi))
    return box


def overlap_counts(slot_a, nvox_a, slot_b, nvox_b, off, n_a, n_b):
    """``(pair [n_a, n_b], in_a [n_a], in_b [n_b])`` int64."""
    pair, in_a, in_b = np.zeros((n_a, n_b), np.int64), np.zeros(n_a, np.int64), np.zeros(n_b, np.int64)
    box = overlap_box(nvox_a, nvox_b, off)
    if box is None:
        return pair, in_a, in_b
    a = np.asarray(slot_a).reshape(nvox_a)[tuple(slice(lo + int(o), hi + int(o)) for (lo, hi), o in zip(box, off))].reshape(-1).astype(np.int64)
    b = np.asarray(slot_b).reshape(nvox_b)[tuple(slice(lo, hi) for lo, hi in box)].reshape(-1).astype(np.int64)
    ma, mb = (a >= 0) & (a < n_a), (b >= 0) & (b < n_b)
    np.add.at(in_a, a[ma], 1)
    np.add.at(in_b, b[mb], 1)
    both = ma & mb
    np.add.at(pair, (a[both], b[both]), 1)
    return pair, in_a, in_b


def assign(pair, in_a, in_b, count_a, count_b, class_a, class_b, merged_a, cos, iou_min, contain_min, cos_min, size_ratio_min):
    """``(match_of_b, kind_of_b)``: 0 new, 1 kept, 2 absorbed, 3 moved.  fp64 comparisons; ties to the smaller a, then b."""
    n_a, n_b = len(in_a), len(in_b)
    match, kind = [-1] * n_b, [0] * n_b
    used_a, used_b = set(), set()
    # 1. absorb: merged a only
    for b in range(n_b):
        best = None
        for a in range(n_a):
            p = int(pair[a][b])
            if merged_a[a] and p > 0 and float(p) >= float(contain_min) * float(in_b[b]):
                if best is None or p > int(pair[best][b]):
                    best = a
        if best is not None:
            match[b], kind[b] = best, 2
            used_b.add(b)
    used_a.update(match[b] for b in used_b)
    # 2. in place
    cand = []
    for a in range(n_a):
        for b in range(n_b):
            p = int(pair[a][b])
            union = float(in_a[a]) + float(in_b[b]) - float(p)
            if a not in used_a and b not in used_b and p > 0 and float(p) >= float(iou_min) * union:
                cand.append((-(float(p) / union), a, b))
    for _, a, b in sorted(cand):
        if a not in used_a and b not in used_b:
            match[b], kind[b] = a, 1
            used_a.add(a)
            used_b.add(b)
    # 3. moved
    cand = []
    for a in range(n_a):
        for b in range(n_b):
            small, large = min(float(count_a[a]), float(count_b[b])), max(float(count_a[a]), float(count_b[b]))
            if a not in used_a and b not in used_b and int(class_a[a]) == int(class_b[b]) and float(cos[a][b]) >= float(cos_min) and \
                    small >= float(size_ratio_min) * large:
                cand.append((-float(cos[a][b]), a, b))
    for _, a, b in sorted(cand):
        if a not in used_a and b not in used_b:
            match[b], kind[b] = a, 3
            used_a.add(a)
            used_b.add(b)
    return np.array(match, dtype=np.int64), np.array(kind, dtype=np.int64)
