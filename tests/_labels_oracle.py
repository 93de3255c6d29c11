"""Numpy restatement of ``ld_draw_labels`` (csrc/eval_image.hip), the exact
arithmetic of include/ld_hip.h:

* a label is ``len * 6 * scale`` by ``8 * scale`` pixels, ``len`` clamped to
  ``0..MAX_LEN``; its corner is ``(x1, y1 - 8 * scale)`` when that row is
  ``>= 0``, else ``(x1, y1)``;
* pixel ``(x, y)`` of it lies in cell column ``cx = (x - x0) // scale``, row
  ``cy = (y - y0) // scale``; character ``cx // 6``, glyph column
  ``gx = cx % 6``; the glyph occupies columns 1-5 and rows 1-7 of the cell, so
  the pixel is foreground iff ``gx >= 1 and cy >= 1`` and bit ``5 - gx`` of
  font row ``cy - 1`` is set; a byte outside 0x20-0x7E takes the glyph of ``?``;
* labels are painted in index order, pixels outside the image are dropped.

The font is the Python-side copy, ``ld_amd.font5x7.FONT``.
"""
import numpy as np

from ld_amd import font5x7 as F


def glyph_cell(c):
    """The 8 x 6 boolean cell of byte ``c``."""
    if c < F.FIRST or c > F.LAST:
        c = ord('?')
    cell = np.zeros((F.CELL_H, F.CELL_W), bool)
    for r in range(F.ROWS):
        bits = int(F.FONT[c - F.FIRST, r])
        for gx in range(1, F.CELL_W):
            cell[r + 1, gx] = bool((bits >> (F.CELL_W - 1 - gx)) & 1)
    return cell


def label_patch(raw, scale):
    """(8 * scale, len * 6 * scale) boolean foreground mask of ``raw``."""
    raw = bytes(raw)[:F.MAX_LEN]
    cells = [glyph_cell(c) for c in raw]
    if not cells:
        return np.zeros((F.CELL_H * scale, 0), bool)
    m = np.concatenate(cells, axis=1)
    return np.repeat(np.repeat(m, scale, axis=0), scale, axis=1)


def draw_labels(img, texts, xy, scale=1, fg=(255, 255, 255), bg=(0, 0, 0)):
    """-> a painted COPY of the (H, W, 3) uint8 ``img``."""
    out = np.array(img, np.uint8, copy=True)
    H, W = out.shape[:2]
    fg, bg = np.asarray(fg, np.uint8), np.asarray(bg, np.uint8)
    for t, (x1, y1) in zip(texts, xy):
        raw = t if isinstance(t, (bytes, bytearray)) else \
            str(t).encode('latin-1', 'replace')
        patch = label_patch(raw, scale)
        h, w = patch.shape
        x0, y0 = int(x1), int(y1) - h if int(y1) - h >= 0 else int(y1)
        for py in range(h):
            y = y0 + py
            if y < 0 or y >= H:
                continue
            for px in range(w):
                x = x0 + px
                if 0 <= x < W:
                    out[y, x] = fg if patch[py, px] else bg
    return out
