"""The reference's BVH build restated in plain numpy float32, from its text alone.

The project has three builders (oracle/mesh_oracle.cpp, the host Builder of pt_mesh.cpp and the device
builder bvh_build.hip) that all come from one reading of BVH_tree.cpp.  This file is a fourth statement of
the same text that shares no code with them: it imports nothing from oracle/ or from the product, works on
whole runs with numpy where they fold element by element, and builds the flattened table directly.  The
rules, each with the lines it comes from (path_tracer/src/ of the reference):

  * Triangle box: glm::min(glm::min(v0, v1), v2) and the same with max, per axis (sceneStructs.h:128-143).
    Centre: 0.5f * (min + max) (BVH_tree.h:19-20).
  * glm::min(x, y) = x < y ? x : y and glm::max(x, y) = x > y ? x : y (glm/detail/func_common.inl:413,
    :434).  boundingbox.h:53-60 and :68-69 pass the NEW value as x, so a tie keeps the OLD one.  Folded
    over a run this is the first of equal values, bits included: +0 and -0 are equal, and the earlier one
    survives.  `_first` states exactly that.
  * `||` on boxes (boundingbox.h:46-63): when `this` is all-zero (==, so -0 counts) the result is the other
    box, untouched.  A fold therefore starts at the first box that is not all-zero, later all-zero boxes
    are unioned as zeros, and a run of only all-zero boxes yields its last box.  (Once the accumulated box
    is not all-zero it stays so: some min is negative or some max is positive, and neither can return to
    0.)  `|| point` (boundingbox.h:65-71) has no such rule.
  * The range fold starts from bb[start] and visits start again (BVH_tree.cpp:35-38); the centre box
    starts from the first centre (:48-51).  The OpenMP pragmas are read as sequential loops.
  * longest_axis (boundingbox.h:20-25), area = 2 * ((dx * dy + dx * dz) + dy * dz) (:32-36) and
    getOffsetBoxes, which divides only where max > min (:94-104).
  * Bucket (BVH_tree.cpp:79-81): (int)(7 * offset), the product in float32, truncation, then 7 -> 6.
  * Cost i (:87-101): counts and `||` folds of the buckets j < i and of the buckets j > i, each from an
    all-zero box, so the boxes of empty buckets are unioned as zeros once the fold is not all-zero;
    1.0f * (c0 * A0 + c1 * A1) / area(bounds), the counts converted to float, no contraction.
  * Split (:103-110): strict < against FLT_MAX, so a NaN or an infinite cost never wins and split_idx
    stays 0.  A cost leaf when min_cost >= n and n <= 8 (:112-119).
  * n == 2 (:63-66): libstdc++'s nth_element on two elements is an insertion sort: swap exactly when the
    second centre < the first.  mid = (int)(1.0f * (start + end) / 2.0f).
  * Otherwise libstdc++'s bidirectional std::partition (:121-128; bits/stl_algo.h __partition): the k-th
    failing element from the left is swapped with the k-th passing element from the right while the left
    one is left of the right one.  mid = start + the number of passing elements, kept in a float.
  * A leaf where the centre box has no extent on its longest axis (:53-60), and at n == 1 (:40-46).
  * An inner node's box is left.bbox || right.bbox (BVH_tree.h:45-51), not the range fold.
  * traverse_bvh (:138-154): preorder, left child at i + 1.  The explicit stack below visits ranges in the
    recursion's order (node, left subtree, right subtree), so a node's creation index is its flattened one.
  * Leaves carry axis = -1 and rchild_idx = -1, inner nodes first_area_idx = 0.  These three are the
    PROJECT'S choice: traverse_bvh leaves them unwritten in a `new BVHTree[]`, so the reference has no
    value for them.

`variant` names one deliberate error, for the sensitivity test: VARIANTS.
"""
from __future__ import annotations

import numpy as np

NODE_DTYPE = np.dtype([("bmin", "<f4", (3,)), ("bmax", "<f4", (3,)), ("sub_areas", "<i4"), ("axis", "<i4"),
                       ("first_area_idx", "<i4"), ("rchild_idx", "<i4")])   # class BVHTree (BVH_tree.h:54-61)

VARIANTS = {
    "cost_includes_i": "the cost loop's first side includes bucket i (j <= i)",
    "no_zero_rule": "`||` without the all-zero rule",
    "stable_partition": "a stable partition instead of libstdc++'s swap pairs",
    "no_swap2": "no swap in the two-element nth_element",
    "rint_bucket": "rint instead of truncation for the bucket",
    "inner_from_fold": "an inner node's box taken from the range fold instead of left || right",
    "tie_keeps_new": "min/max ties keep the new value (the last of equal values)",
}

F32 = np.float32
N_REGIONS = 7            # MAX_AREAS - 1 (BVH_tree.cpp:3, :75)
MAX_AREAS = 8
FLT_MAX = np.finfo(np.float32).max
ZERO_BOX = np.zeros((2, 3), np.float32)
_COLUMNS = np.arange(3)


def glm_min(x, y):
    return np.where(x < y, x, y)


def glm_max(x, y):
    return np.where(x > y, x, y)


def triangle_boxes(v):
    """(n, 3, 3) float32 vertices -> (n, 2, 3) boxes [min, max] and (n, 3) centres."""
    v = np.asarray(v, np.float32)
    lo = glm_min(glm_min(v[:, 0], v[:, 1]), v[:, 2])
    hi = glm_max(glm_max(v[:, 0], v[:, 1]), v[:, 2])
    return np.stack([lo, hi], 1), F32(0.5) * (lo + hi)


def _first(a, largest, last=False):
    """acc = a[0]; acc = glm::min(a[i], acc) for the rest (max when `largest`), per column: the first of the
    equal extreme values.  np.argmin / np.argmax return the first occurrence and compare +0 == -0.
    last=True is the deliberate error 'tie_keeps_new'."""
    pick = np.argmax if largest else np.argmin
    idx = len(a) - 1 - pick(a[::-1], axis=0) if last else pick(a, axis=0)
    return a[idx, _COLUMNS]


def fold_boxes(seq, variant=None):
    """acc = seq[0]; acc = acc || seq[i] for the rest (boundingbox.h:46-63).  seq: (k, 2, 3)."""
    last = variant == "tie_keeps_new"
    if variant != "no_zero_rule":
        nonzero = (seq != 0.0).reshape(len(seq), 6).any(axis=1)
        if not nonzero.any():
            return seq[-1].copy()
        seq = seq[nonzero.argmax():]
    return np.stack([_first(seq[:, 0], False, last), _first(seq[:, 1], True, last)])


def fold_from_zero(seq, variant=None):
    """acc = BoundingBox(); acc = acc || seq[i] for all of seq: the all-zero start hands over to seq[0]."""
    if variant == "no_zero_rule":
        return fold_boxes(np.concatenate([ZERO_BOX[None], seq]), variant)
    return fold_boxes(seq, variant) if len(seq) else ZERO_BOX.copy()


def area(b):
    d = b[1] - b[0]
    return F32(2.0) * ((d[0] * d[1] + d[0] * d[2]) + d[1] * d[2])


def longest_axis(b):
    d = b[1] - b[0]
    return 0 if (d[0] > d[1] and d[0] > d[2]) else (1 if d[1] > d[2] else 2)


def buckets(cb, c, axis, variant=None):
    """(int)(n_regions * getOffsetBoxes(c)[axis]), 7 -> 6, for a run of centres."""
    off = c[:, axis] - cb[0, axis]
    if cb[1, axis] > cb[0, axis]:
        off = off / (cb[1, axis] - cb[0, axis])
    f = F32(N_REGIONS) * off
    idx = (np.rint(f) if variant == "rint_bucket" else np.trunc(f)).astype(np.int32)
    idx[idx == N_REGIONS] = N_REGIONS - 1
    return idx


def partition_swaps(passing):
    """libstdc++'s bidirectional std::partition as the swaps it makes, for a boolean run: index pairs
    (left, right).  The k-th failing from the left meets the k-th passing from the right."""
    fail_left = np.flatnonzero(~passing)
    pass_right = np.flatnonzero(passing)[::-1]
    k = min(len(fail_left), len(pass_right))
    keep = fail_left[:k] < pass_right[:k]
    return fail_left[:k][keep], pass_right[:k][keep]


def partition_literal(passing):
    """bits/stl_algo.h __partition(first, last, pred, bidirectional_iterator_tag), statement for statement,
    on a boolean run; returns (the permutation it leaves, the split point).  partition_swaps is checked
    against it by the CPU test."""
    p = list(passing)
    perm = list(range(len(p)))
    first, last = 0, len(p)
    while True:
        while True:
            if first == last:
                return perm, first
            if p[first]:
                first += 1
            else:
                break
        last -= 1
        while True:
            if first == last:
                return perm, first
            if not p[last]:
                last -= 1
            else:
                break
        p[first], p[last] = p[last], p[first]
        perm[first], perm[last] = perm[last], perm[first]
        first += 1


def sah_split(run, idx, bounds, variant=None):
    """BVH_tree.cpp:75-110 for a run of boxes with their buckets: (min_cost, split_idx)."""
    count = np.bincount(idx, minlength=N_REGIONS).tolist()
    rb = np.stack([fold_from_zero(run[idx == r], variant) for r in range(N_REGIONS)])
    min_cost, split_idx = FLT_MAX, 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        total = area(bounds)
        for i in range(N_REGIONS - 1):
            lo_end = i + 1 if variant == "cost_includes_i" else i
            c0, c1 = sum(count[:lo_end]), sum(count[i + 1:])
            a0, a1 = fold_from_zero(rb[:lo_end], variant), fold_from_zero(rb[i + 1:], variant)
            cost = F32(1.0) * (F32(c0) * area(a0) + F32(c1) * area(a1)) / total
            if cost < min_cost:
                min_cost, split_idx = cost, i
    return min_cost, split_idx


def build(v, variant=None):
    """build_bvh_tree (BVH_tree.cpp:156-181) of the load-order vertices (n, 3, 3): the flattened nodes
    (NODE_DTYPE) and the leaf order as load indices (triangles.swap(ordered_triangles))."""
    assert variant is None or variant in VARIANTS, variant
    v = np.asarray(v, np.float32)
    n = len(v)
    if n == 0:
        return np.zeros(0, NODE_DTYPE), np.zeros(0, np.int64)
    assert np.isfinite(v).all()
    bb, centre = triangle_boxes(v)
    index = np.arange(n)                     # BVH_BBox::index, permuted in place with bb and centre
    ordered = []                             # ordered_triangles, as load indices
    box, axis_of, count_of, first_of, rchild = [], [], [], [], []
    tie_last = variant == "tie_keeps_new"

    def leaf(start, end, bounds):            # mkLeaf (BVH_tree.h:39-44)
        first_of.append(len(ordered))
        ordered.extend(index[start:end].tolist())
        box.append(bounds)
        axis_of.append(-1)
        count_of.append(end - start)
        rchild.append(-1)

    stack = [(0, n, -1)]                     # (start, end, the parent whose right child this is, or -1)
    while stack:
        start, end, parent = stack.pop()
        me = len(box)                        # n_nodes += 1
        if parent >= 0:
            rchild[parent] = me
        n_tris = end - start
        bounds = fold_boxes(np.concatenate([bb[start:start + 1], bb[start:end]]), variant)
        if n_tris == 1:
            leaf(start, end, bounds)
            continue
        c = np.concatenate([centre[start:start + 1], centre[start:end]])
        central = np.stack([_first(c, False, tie_last), _first(c, True, tie_last)])
        c = centre[start:end]
        axis = longest_axis(central)
        if central[0, axis] == central[1, axis]:
            leaf(start, end, bounds)
            continue
        if n_tris == 2:
            mid = int(F32(1.0) * F32(start + end) / F32(2.0))
            if centre[start + 1, axis] < centre[start, axis] and variant != "no_swap2":
                for arr in (bb, centre, index):
                    arr[start:end] = arr[[start + 1, start]]
        else:
            idx = buckets(central, c, axis, variant)
            min_cost, split_idx = sah_split(bb[start:end], idx, bounds, variant)
            if min_cost >= F32(n_tris) and n_tris <= MAX_AREAS:
                leaf(start, end, bounds)
                continue
            passing = idx <= split_idx
            if variant == "stable_partition":
                perm = np.concatenate([np.flatnonzero(passing), np.flatnonzero(~passing)])
            else:
                left, right = partition_swaps(passing)
                perm = np.arange(n_tris)
                perm[left], perm[right] = right, left
            for arr in (bb, centre, index):
                arr[start:end] = arr[start:end][perm]
            mid = int(F32(start + int(passing.sum())))   # `float mid` (BVH_tree.cpp:62, :128)
        assert start < mid < end, "a split left one side empty: the reference would recurse without end"
        box.append(bounds)                   # mkNode replaces it by left || right, below
        axis_of.append(axis)
        count_of.append(0)
        first_of.append(0)
        rchild.append(-1)
        stack.append((mid, end, me))         # popped after the whole left subtree
        stack.append((start, mid, -1))
    nodes = np.zeros(len(box), NODE_DTYPE)
    for i in range(len(box) - 1, -1, -1):    # mkNode: children are made first; their indices are larger
        if count_of[i] == 0 and variant != "inner_from_fold":
            box[i] = fold_boxes(np.stack([box[i + 1], box[rchild[i]]]), variant)
    boxes = np.stack(box)
    nodes["bmin"], nodes["bmax"] = boxes[:, 0], boxes[:, 1]
    nodes["sub_areas"], nodes["axis"] = count_of, axis_of
    nodes["first_area_idx"], nodes["rchild_idx"] = first_of, rchild
    return nodes, np.asarray(ordered, np.int64)


def first_difference(a, b):
    """A line that names the first differing node of two node tables, for assertion messages."""
    if len(a) != len(b):
        return f"{len(a)} nodes vs {len(b)} nodes"
    ra = np.frombuffer(a.tobytes(), np.uint8).reshape(len(a), -1)
    rb = np.frombuffer(b.tobytes(), np.uint8).reshape(len(b), -1)
    bad = np.flatnonzero((ra != rb).any(axis=1))
    if len(bad) == 0:
        return "no difference"
    i = int(bad[0])
    return f"{len(bad)} of {len(a)} nodes differ, the first is node {i}: {a[i]} vs {b[i]}"
