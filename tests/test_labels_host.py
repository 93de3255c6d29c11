"""CPU checks of the label painter's host side: the kernel's font table
(csrc/font5x7.h, read back through ``ld_font_glyph``) equals the Python copy
(ld_amd/font5x7.py); the numpy oracle (tests/_labels_oracle.py) gives the
hand-drawn bitmaps of 'A', '|' and '0'; ``ld_draw_labels`` rejects bad
arguments before any launch; the label text is the reference's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _labels_oracle as LO  # noqa: E402

from ld_amd import font5x7 as F  # noqa: E402


def _art(rows):
    return np.array([[ch == '#' for ch in r] for r in rows], bool)


# drawn by hand on squared paper: 6 x 8 cells, glyph at columns 1-5, rows 1-7
A_CELL = _art(['......',
               '..###.',
               '.#...#',
               '.#...#',
               '.#...#',
               '.#####',
               '.#...#',
               '.#...#'])
BAR_CELL = _art(['......',
                 '...#..',
                 '...#..',
                 '...#..',
                 '...#..',
                 '...#..',
                 '...#..',
                 '...#..'])
ZERO_CELL = _art(['......',
                  '..###.',
                  '.#...#',
                  '.#..##',
                  '.#.#.#',
                  '.##..#',
                  '.#...#',
                  '..###.'])


def test_font_table_c_equals_python():
    from ld_amd import lib as L
    lib = L.get_lib()
    assert F.FONT.shape == (95, 7) and F.FONT.dtype == np.uint8
    assert int(F.FONT.max()) < 32  # five columns
    for c in range(F.FIRST, F.LAST + 1):
        for r in range(F.ROWS):
            assert lib.ld_font_glyph(c, r) == int(F.FONT[c - F.FIRST, r]), \
                (chr(c), r)
    for c, r in ((F.FIRST - 1, 0), (F.LAST + 1, 0), (-1, 0), (256, 0),
                 (ord('A'), -1), (ord('A'), F.ROWS)):
        assert lib.ld_font_glyph(c, r) == -1
    # every printable character but the space has ink, and no two look alike
    assert (F.FONT[1:].sum(axis=1) > 0).all() and F.FONT[0].sum() == 0
    assert len({bytes(g) for g in F.FONT}) == 95


def test_oracle_known_glyphs():
    np.testing.assert_array_equal(LO.glyph_cell(ord('A')), A_CELL)
    np.testing.assert_array_equal(LO.glyph_cell(ord('|')), BAR_CELL)
    np.testing.assert_array_equal(LO.glyph_cell(ord('0')), ZERO_CELL)
    np.testing.assert_array_equal(LO.glyph_cell(0x7F),
                                  LO.glyph_cell(ord('?')))
    np.testing.assert_array_equal(LO.glyph_cell(0x1F),
                                  LO.glyph_cell(ord('?')))


def test_oracle_known_label():
    """'A|0' at scale 1 above y1 = 10, and the same at scale 2 flipped below
    y1 = 3 and clipped at the right border."""
    img = np.full((20, 30, 3), 7, np.uint8)
    fg, bg = (1, 2, 3), (250, 251, 252)
    out = LO.draw_labels(img, ['A|0'], [(4, 10)], 1, fg, bg)
    want = img.copy()
    cells = np.concatenate([A_CELL, BAR_CELL, ZERO_CELL], axis=1)
    want[2:10, 4:22] = np.where(cells[..., None], np.uint8(fg), np.uint8(bg))
    np.testing.assert_array_equal(out, want)
    out = LO.draw_labels(img, ['A|0'], [(4, 3)], 2, fg, bg)
    want = img.copy()
    big = np.repeat(np.repeat(cells, 2, axis=0), 2, axis=1)  # 16 x 36
    want[3:19, 4:30] = np.where(big[:, :26, None], np.uint8(fg), np.uint8(bg))
    np.testing.assert_array_equal(out, want)
    # an empty text paints nothing; a later label paints over an earlier one
    np.testing.assert_array_equal(LO.draw_labels(img, [''], [(4, 10)]), img)
    two = LO.draw_labels(img, ['AA', '0'], [(0, 8), (3, 8)], 1, fg, bg)
    np.testing.assert_array_equal(
        two[0:8, 3:9], np.where(ZERO_CELL[..., None], np.uint8(fg),
                                np.uint8(bg)))
    np.testing.assert_array_equal(
        two[0:8, 0:3], np.where(A_CELL[:, :3, None], np.uint8(fg),
                                np.uint8(bg)))


def test_draw_labels_argument_validation_without_gpu():
    from ld_amd import lib as L
    lib = L.get_lib()
    assert lib.ld_draw_labels(None, 0, 5, None, None, 3, 1, 0, 0, None) == 0
    assert lib.ld_draw_labels(None, 5, 5, None, None, 0, 1, 0, 0, None) == 0
    assert lib.ld_draw_labels(None, -1, 5, None, None, 1, 1, 0, 0, None) == -1
    assert lib.ld_draw_labels(None, 5, -1, None, None, 1, 1, 0, 0, None) == -1
    assert lib.ld_draw_labels(None, 5, 5, None, None, -1, 1, 0, 0, None) == -1
    assert lib.ld_draw_labels(None, 5, 5, None, None, 1, 0, 0, 0, None) == -1
    assert lib.ld_draw_labels(None, 5, 5, None, None, 1, 1, 0, 0, None) == -1
    assert lib.ld_draw_labels(None, 5, 5, None, None, 0, 0, 0, 0, None) == -1


def test_label_texts_and_cpu_refusal():
    import torch
    from ld_amd import analyze_results as A
    dets = np.array([[1, 2, 3, 4, 0.125], [1, 2, 3, 4, 0.999]], np.float32)
    assert A.label_texts(dets, [1, 0], ('cat', 'dog')) == \
        ['dog|0.12', 'cat|1.00']
    assert A.label_texts(dets[:1], [5], ('cat', 'dog')) == ['cls 5|0.12']
    assert A.label_texts(dets[:1], [0], None) == ['cls 0|0.12']
    with pytest.raises(L_error()):
        A.draw_labels(torch.zeros(4, 4, 3, dtype=torch.uint8), ['a'], [(0, 0)])


def L_error():
    from ld_amd import lib as L
    return L.LdError
