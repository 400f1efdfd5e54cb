"""NumPy model of a mesh refit (include/rtgpu.h, rtgpu_update_mesh): the triangle, box and gate rules, operation for operation.

  triangle t, vertex indices i0 i1 i2:  v0 = P[i0], edge1 = P[i1] - P[i0], edge2 = P[i2] - P[i0] (float32, one subtraction per lane);
                                        its box = Min(a, Min(b, c)), Max(a, Max(b, c)) of the three POSITIONS, Min(a, b) = a < b ? a : b
  a leaf                                its triangles' boxes joined first to last: Box(box0, box1) = Min(box0.min, box1.min), Max(box0.max, box1.max)
  an interior node                      Box(child0, child1)
  node 1, childIndex, leaves            untouched
  gates                                 gate[2 p], gate[2 p + 1] = {min, 0}, {max, 0} of the leaf whose first triangle is p; zero elsewhere

Everything is float32 and every result is one of its inputs or one rounded subtraction, so the model pins the tables bit for bit.  The fold ORDER is part
of the rule (it decides the sign of a zero); meshes in the tests are jittered so that no coordinate is zero and the order cannot hide."""
import numpy as np


def _min(a, b):
    return np.where(a < b, a, b)


def _max(a, b):
    return np.where(a > b, a, b)


def triangles_of(indices, positions):
    """(T, 9) float32 records and the (T, 3) min / max of the triangles' boxes; indices: (T, >= 3) vertex indices in leaf order."""
    p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    a, b, c = p[indices[:, 0]], p[indices[:, 1]], p[indices[:, 2]]
    records = np.concatenate([a, b - a, c - a], axis=1).astype(np.float32)
    return records, _min(a, _min(b, c)), _max(a, _max(b, c))


def refit(nodes, indices, positions):
    """nodes: (N, 8) uint32 words (min.xyz, childIndex, max.xyz, leaves) in any order with their own child indices.  Returns (nodes, triangles, gates):
    the refitted node words, the (T, 9) float32 triangle records and the (2 T, 4) float32 gate records."""
    nodes = np.array(nodes, dtype=np.uint32, copy=True)
    indices = np.asarray(indices, dtype=np.uint32)
    records, lo, hi = triangles_of(indices, positions)
    gates = np.zeros((2 * len(indices), 4), dtype=np.float32)
    if len(nodes) == 0 or len(indices) == 0:
        return nodes, records, gates
    boxes = nodes.view(np.float32)     # words 0..2 and 4..6
    stack = [(0, False)]
    while stack:
        n, children_done = stack.pop()
        first, leaves = int(nodes[n, 3]), int(nodes[n, 7]) & 0x3FFFFFFF
        if leaves:
            bmin, bmax = lo[first], hi[first]
            for j in range(1, leaves):
                bmin, bmax = _min(bmin, lo[first + j]), _max(bmax, hi[first + j])
            gates[2 * first, :3], gates[2 * first + 1, :3] = bmin, bmax
        elif not children_done:
            stack += [(n, True), (first + 1, False), (first, False)]
            continue
        else:
            bmin, bmax = _min(boxes[first, 0:3], boxes[first + 1, 0:3]), _max(boxes[first, 4:7], boxes[first + 1, 4:7])
        boxes[n, 0:3], boxes[n, 4:7] = bmin, bmax
    return nodes, records, gates


def depth_widths(nodes):
    """Number of nodes at every depth of the tree (root = depth 0): which depths a refit walks in one block and which get a launch of their own."""
    widths, level = [], [0]
    while level:
        widths.append(len(level))
        level = [c for n in level if not int(nodes[n, 7]) & 0x3FFFFFFF for c in (int(nodes[n, 3]), int(nodes[n, 3]) + 1)]
    return widths
