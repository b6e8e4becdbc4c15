"""Frames of a recorded episode (runtime.Episode, from EvalBatch.recording) as RGB arrays: the reference's
``render_mode="rgb_array"`` and the per-decision images of ``DistrQLearning.test(plot=True)`` (distr_q.py:216-221).

A pure-numpy integer rasteriser: no fonts, no anti-aliasing, no floating point, so a frame is the same array on every
machine.  A map cell is a ``cell_px`` x ``cell_px`` square.  ``rail_image`` draws what does not change: the rails from
the 16-bit transition grid (a stroke from the cell's centre to the middle of every side a train can enter or leave it
through), switch cells on a tinted ground and target cells with a corner mark.  ``frame`` adds the trains of one
recorded tick: a filled square in the train's own colour (``train_colour``, fixed per handle) with a dark tick towards
its heading, the cell's border in ``MALFUNCTION`` when the train is in that state, and the border of a decision's
switch cell in ``DECIDING``.  A train off the map paints nothing.  ``save_png`` is the only function that needs an
image library."""
from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np

from .compiler import CompiledMap
from .mapgen import transitions

BACKGROUND = (255, 255, 255)
RAIL = (96, 96, 96)
SWITCH = (222, 228, 240)
TARGET = (255, 200, 0)
HEADING = (0, 0, 0)
MALFUNCTION = (255, 0, 0)
DECIDING = (255, 0, 255)
S_MALFUNCTION = 5  # _lib.TRAIN_STATES
_RESERVED = (BACKGROUND, RAIL, SWITCH, TARGET, HEADING, MALFUNCTION, DECIDING)
MAX_TRAINS = 128


def train_colour(h: int) -> Tuple[int, int, int]:
    """The marker colour of train handle ``h``: fixed, distinct for every handle below 128, none of the colours above."""
    return _PALETTE[int(h)]


def _palette():
    out, seen = [], set(_RESERVED)
    x = 1
    while len(out) < MAX_TRAINS:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        c = (32 + (x >> 4) % 192, 32 + (x >> 12) % 192, 32 + (x >> 20) % 192)
        # (mid-range channels: never the white ground, the black tick or the saturated marks; not a grey like the rails)
        if c not in seen and max(c) - min(c) >= 48:
            seen.add(c)
            out.append(c)
    return tuple(out)


_PALETTE = _palette()


def _check_px(cell_px: int) -> int:
    px = int(cell_px)
    if px < 4:
        raise ValueError("render: cell_px is at least 4")
    return px


def _border(img: np.ndarray, r: int, c: int, px: int, colour) -> None:
    y, x = r * px, c * px
    img[y, x:x + px] = colour
    img[y + px - 1, x:x + px] = colour
    img[y:y + px, x] = colour
    img[y:y + px, x + px - 1] = colour


def rail_image(cm: CompiledMap, cell_px: int = 8) -> np.ndarray:
    """uint8 [H * px][W * px][3]: the rails, the switch cells and the target cells of the map."""
    px = _check_px(cell_px)
    H, W = cm.H, cm.W
    img = np.empty((H * px, W * px, 3), np.uint8)
    img[:] = BACKGROUND
    for r, c in cm.switch_ids:
        img[r * px:(r + 1) * px, c * px:(c + 1) * px] = SWITCH
    grid = cm.arrays["grid"].reshape(H, W)
    m = px // 2
    for r, c in zip(*np.nonzero(grid)):
        w = int(grid[r, c])
        sides = set()
        for heading in range(4):
            ex = transitions(w, heading)
            if any(ex):
                sides.add((heading + 2) % 4)  # entered through the side opposite to the heading
                sides.update(e for e in range(4) if ex[e])
        y, x = int(r) * px, int(c) * px
        for s in sides:  # N, E, S, W
            if s == 0:
                img[y:y + m + 1, x + m] = RAIL
            elif s == 1:
                img[y + m, x + m:x + px] = RAIL
            elif s == 2:
                img[y + m:y + px, x + m] = RAIL
            else:
                img[y + m, x:x + m + 1] = RAIL
    k = max(px // 4, 1)
    for t in cm.arrays["tr_target"]:
        r, c = divmod(int(t), W)
        img[r * px:r * px + k, c * px:c * px + k] = TARGET
    return img


def frame(cm: CompiledMap, episode, t: int, decision: Optional[int] = None, cell_px: int = 8) -> np.ndarray:
    """uint8 [H * px][W * px][3]: the map with the trains as they stand in frame ``t`` of the episode (after tick
    t + 1); ``decision``: a row of the episode whose deciding switch is highlighted."""
    px = _check_px(cell_px)
    img = rail_image(cm, px)
    if decision is not None:
        r, c = cm.switch_ids[int(episode.decisions["switch"][int(decision)])]
        _border(img, int(r), int(c), px, DECIDING)
    cell, heading, state = episode.cell[t], episode.heading[t], episode.state[t]
    lo, hi, m = px // 4, px - px // 4, px // 2
    for h in range(len(cell)):
        if cell[h] < 0:
            continue
        r, c = divmod(int(cell[h]), cm.W)
        y, x = r * px, c * px
        img[y + lo:y + hi, x + lo:x + hi] = train_colour(h)
        d = int(heading[h])
        if d == 0:
            img[y + lo:y + m, x + m] = HEADING
        elif d == 1:
            img[y + m, x + m + 1:x + hi] = HEADING
        elif d == 2:
            img[y + m + 1:y + hi, x + m] = HEADING
        else:
            img[y + m, x + lo:x + m] = HEADING
        if int(state[h]) == S_MALFUNCTION:
            _border(img, r, c, px, MALFUNCTION)
    return img


def frames_at_decisions(cm: CompiledMap, episode, cell_px: int = 8) -> Iterator[np.ndarray]:
    """One frame per recorded decision, as the trains stand when its step returned (``step_now``), with its switch
    highlighted: the reference's one image per iteration.  A ``step_now`` past the kept frames shows the last one."""
    for d in range(episode.rows):
        t = min(max(int(episode.decisions["step_now"][d]) - 1, 0), episode.frames - 1)
        yield frame(cm, episode, t, decision=d, cell_px=cell_px)


def save_png(path, rgb: np.ndarray) -> None:
    """Write an RGB array as a PNG with PIL or, without it, matplotlib; neither present is an error."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        Image.fromarray(rgb).save(str(path), format="PNG")
        return
    try:
        from matplotlib.image import imsave
    except ImportError:
        raise RuntimeError("render.save_png needs PIL (Pillow) or matplotlib to write a PNG; neither is installed")
    imsave(str(path), rgb, format="png")
