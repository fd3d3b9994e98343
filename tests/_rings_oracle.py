"""The polygon rings of include/gdlhip_scene_rings.h restated in numpy and plain Python, the yardstick of
tests/test_scene_rings_host.py and tests/test_hip_scene_rings.py.

``successor``: the header's successor rule over all 4 * H * W slots at once.  ``trace``: a sequential tracer that walks it side by
side from every unvisited boundary side in slot order (so a ring starts at its smallest slot and the rings come by ascending
start), emits a vertex at every corner side and adds up the shoelace sum over the vertices.  ``fill``: the inverse, from the
rings back to the label image by the unit vertical steps of the rings alone."""

from typing import NamedTuple

import numpy as np

import _sieve_oracle as so

# d_s, the direction of travel of side s, as (dy, dx): E, S, W, N; the outward normal n_s is d_{(s + 3) % 4}
STEP = ((0, 1), (1, 0), (0, -1), (-1, 0))
# the head point of side s of pixel (y, x) is (x + HEAD[s][0], y + HEAD[s][1])
HEAD = ((1, 0), (1, 1), (0, 1), (0, 0))


class Rings(NamedTuple):      # the fields of gdlhip.ops.SceneRings, as numpy arrays
    vertices: np.ndarray      # int32 [V, 2]
    ring_offsets: np.ndarray  # int32 [R + 1]
    value: np.ndarray         # uint8 [R]
    label: np.ndarray         # int32 [R]
    start: np.ndarray         # int32 [R]
    area2: np.ndarray         # int64 [R]


def live_pixels(mask: np.ndarray, ignore_label: int = -1, values=None) -> np.ndarray:
    live = mask != ignore_label
    return live if values is None else live & np.isin(mask, list(values))


def successor(mask: np.ndarray, connectivity: int = 4, ignore_label: int = -1, values=None):
    """(boundary bool [4 * H * W], next int64 [4 * H * W]) by slot; next is -1 where the slot is no boundary side."""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity {connectivity}")
    H, W = mask.shape
    live = live_pixels(mask, ignore_label, values)
    padded = np.full((H + 2, W + 2), -1, dtype=np.int16)      # -1: outside the raster, equal to no pixel
    padded[1:-1, 1:-1] = mask

    def same(dy: int, dx: int) -> np.ndarray:      # the pixel at p + (dy, dx) is inside and has p's value
        return padded[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == mask

    p = np.arange(H * W, dtype=np.int64).reshape(H, W)
    boundary, nxt = np.zeros((H, W, 4), dtype=bool), np.full((H, W, 4), -1, dtype=np.int64)
    for s in range(4):
        (dy, dx), (ny, nx) = STEP[s], STEP[(s + 3) % 4]
        boundary[:, :, s] = live & ~same(ny, nx)
        same_a, same_b = same(dy, dx), same(dy + ny, dx + nx)
        turn, to_a, to_b = 4 * p + (s + 1) % 4, 4 * (p + dy * W + dx) + s, 4 * (p + (dy + ny) * W + dx + nx) + (s + 3) % 4
        if connectivity == 4:
            succ = np.where(~same_a, turn, np.where(same_b, to_b, to_a))
        else:
            succ = np.where(same_b, to_b, np.where(same_a, to_a, turn))
        nxt[:, :, s] = np.where(boundary[:, :, s], succ, -1)
    return boundary.reshape(-1), nxt.reshape(-1)


def trace(mask: np.ndarray, connectivity: int = 4, ignore_label: int = -1, values=None, labels=None) -> Rings:
    """``labels``: what ``_sieve_oracle.components`` gives for the mask, connectivity and ignore_label, where the caller has it."""
    H, W = mask.shape
    if labels is None:
        labels = so.components(mask, connectivity, ignore_label)[0]
    boundary, nxt = successor(mask, connectivity, ignore_label, values)
    nxt, visited = nxt.tolist(), bytearray(4 * H * W)
    vertices, offsets, starts, area2 = [], [0], [], []
    for start in np.flatnonzero(boundary).tolist():
        if visited[start]:
            continue
        ring, cur = [], start
        while True:
            visited[cur] = 1
            follow = nxt[cur]
            if follow < 0 or (visited[follow] and follow != start):
                raise ValueError(f"slot {cur} leads to slot {follow}: the successor map is no permutation of the boundary sides")
            if (follow ^ cur) & 3:      # a corner side
                pixel, s = cur >> 2, cur & 3
                ring.append((pixel % W + HEAD[s][0], pixel // W + HEAD[s][1]))
            cur = follow
            if cur == start:
                break
        area2.append(sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:] + ring[:1])))
        vertices += ring
        offsets.append(len(vertices))
        starts.append(start)
    pixels = np.array(starts, dtype=np.int64) >> 2
    return Rings(np.array(vertices, dtype=np.int32).reshape(-1, 2), np.array(offsets, dtype=np.int32),
                 mask.reshape(-1)[pixels].astype(np.uint8), labels.reshape(-1)[pixels].astype(np.int32),
                 np.array(starts, dtype=np.int32), np.array(area2, dtype=np.int64))


def fill(rings, H: int, W: int) -> np.ndarray:
    """int32 [H, W]: the label whose rings enclose the pixel, -1 where none does.  Every unit vertical step of a ring between the
    lattice rows y and y + 1 at the lattice column x adds +1 (going up: the region lies to the east) or -1 (going down) to a
    difference plane of the ring's label at (y, x), and the cumulative sum along x of the label's plane must be its indicator.
    Held per label without a plane each: sorted by (label, y, x) the steps must alternate +1, -1 (the running sum stays in
    {0, 1} and ends every row at 0), so every label's sum is an indicator; then the sum of all indicators must be an indicator
    too, and where it is 1 the sum weighted by label + 1 names the label.  Anything else is a ValueError."""
    v, offsets = np.asarray(rings.vertices, dtype=np.int64), np.asarray(rings.ring_offsets, dtype=np.int64)
    label = np.repeat(np.asarray(rings.label, dtype=np.int64), np.diff(offsets))
    follow = np.arange(len(v)) + 1
    follow[offsets[1:] - 1] = offsets[:-1]      # the ring closes
    x, y0, y1 = v[:, 0], v[:, 1], v[follow, 1]
    vertical = v[follow, 0] == x
    if (vertical == (y0 == y1)).any():
        raise ValueError("a segment that is neither horizontal nor vertical, or of length 0")
    x, y0, y1, label = x[vertical], y0[vertical], y1[vertical], label[vertical]
    length = np.abs(y1 - y0)
    first = np.repeat(np.minimum(y0, y1), length)      # the rows of a segment: min(y0, y1) .. max(y0, y1) - 1
    rows = first + np.arange(length.sum()) - np.repeat(np.cumsum(length) - length, length)
    cols, labs, sign = np.repeat(x, length), np.repeat(label, length), np.repeat(np.where(y1 < y0, 1, -1), length)
    if len(rows) and (rows.min() < 0 or rows.max() >= H or cols.min() < 0 or cols.max() > W):
        raise ValueError("a vertex outside the lattice of the raster")
    order = np.lexsort((cols, rows, labs))
    run = np.cumsum(sign[order])
    last = np.ones(len(order), dtype=bool)      # the last step of every (label, row)
    last[:-1] = (labs[order][1:] != labs[order][:-1]) | (rows[order][1:] != rows[order][:-1])
    if len(run) and (run.min() < 0 or run.max() > 1 or run[last].any()):
        raise ValueError("the vertical steps of a label do not alternate up, down along a row")
    cover, weighted = np.zeros((H, W + 1), dtype=np.int64), np.zeros((H, W + 1), dtype=np.int64)
    np.add.at(cover, (rows, cols), sign)
    np.add.at(weighted, (rows, cols), sign * (labs + 1))
    cover, weighted = np.cumsum(cover, axis=1)[:, :W], np.cumsum(weighted, axis=1)[:, :W]
    if cover.min(initial=0) < 0 or cover.max(initial=0) > 1:
        raise ValueError("two labels enclose one pixel")
    return np.where(cover == 1, weighted - 1, -1).astype(np.int32)
