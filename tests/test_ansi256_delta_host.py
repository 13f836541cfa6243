"""The delta texts in the xterm 256-colour palette as the sequential host emitters state them (trt_emitter_delta256_rgb8,
trt_emitter_delta256_half_rgb8; csrc/host/trt_emit.c), without a GPU: a model of a terminal that has been sent the whole palette text of a
frame and then the delta shows exactly the search's indices of the next frame; the text's changed cells are a subset of the 24-bit
delta's of the same pair, so it has no more records; the three families that only a palette text has give what they are there to give;
the capacities are those of the format."""
import numpy as np
import pytest

import ansi256_delta_support as A
import ansi_delta_half_support as H
import ansi_delta_support as D
from terminalraytracer_amd import hip, host

SIZES = [(1, 1), (2, 1), (3, 2), (5, 3), (67, 13), (131, 17)]
HALF_IDS = ["full", "half"]


def families(half):
    return A.HALF_FAMILIES if half else A.FAMILIES


def painted_24bit(shown, nxt, half):
    """the cells the 24-bit delta text of the pair paints: bool [cell rows, width], by the 24-bit kind's terminal model"""
    rows, w, _ = shown.shape
    if half:
        return H.Terminal(w, rows).feed(host.emitter_delta_half_rgb8(shown, nxt)).grid[..., 0] != H.NEVER
    return D.Terminal(w, rows).feed(host.emitter_delta_rgb8(shown, nxt)).grid[:, ::2] != D.NEVER


def painted_256(shown, nxt, half):
    rows, w, _ = shown.shape
    term = (A.HalfTerminal if half else A.Terminal)(w, rows).feed(host.emitter_delta256_rgb8(shown, nxt, half))
    cells = np.zeros(term.grid.shape[:2] if half else (rows, w), dtype=bool)
    for r, c in term.records:
        assert not cells[r, c], f"cell ({r}, {c}) has two records"
        cells[r, c] = True
    return cells


def check_pair(shown, nxt, half, what):
    rows, w, _ = shown.shape
    terminal = A.HalfTerminal if half else A.Terminal
    text = host.emitter_delta256_rgb8(shown, nxt, half)
    assert text.size <= A.bound(w, rows, half), what
    term = terminal(w, rows).feed(host.emitter_ansi256_rgb8(shown, half))
    term.shows(shown, f"{what}: the whole text")
    term.feed(text).shows(nxt, f"{what}: the delta behind it")
    ours, theirs = painted_256(shown, nxt, half), painted_24bit(shown, nxt, half)
    assert not (ours & ~theirs).any(), f"{what}: a cell of the palette delta that the 24-bit delta leaves alone"
    assert ours.sum() <= theirs.sum(), what
    changed = (A.half_indices(shown) != A.half_indices(nxt)).any(axis=2) if half else A.indices(shown) != A.indices(nxt)
    assert np.array_equal(ours, changed), f"{what}: the records are not those of the cells whose index changed"
    return text


@pytest.mark.parametrize("half", [False, True], ids=HALF_IDS)
def test_a_terminal_that_shows_the_whole_text_and_is_sent_the_delta_shows_the_next_frame(half):
    for family in families(half):
        for w, rows in SIZES:
            shown, nxt = A.pair(family, w, rows, half=half)
            text = check_pair(shown, nxt, half, f"{family} {w}x{rows}")
            if family == "nothing":
                assert text.size == 0


@pytest.mark.parametrize("half", [False, True], ids=HALF_IDS)
def test_bytes_that_move_inside_a_palette_entry_give_no_text(half):
    """ "same index": every pixel's bytes differ, so the 24-bit delta text is the longest there is for the size; no index does: 0 bytes"""
    for w, rows in SIZES:
        shown, nxt = A.pair("same index", w, rows, half=half)
        assert (shown != nxt).any(axis=2).all()
        assert host.emitter_delta256_rgb8(shown, nxt, half).size == 0
        if half:
            most = H.bound(w, rows) - (17 * (w - 1) if rows % 2 else 0)  # an odd frame's last text row has one lower colour
            assert host.emitter_delta_half_rgb8(shown, nxt).size == most
        else:
            assert host.emitter_delta_rgb8(shown, nxt).size == D.bound(w, rows)


@pytest.mark.parametrize("half", [False, True], ids=HALF_IDS)
def test_neighbours_of_one_index_share_a_colour_whatever_their_bytes(half):
    """ "index run": every cell changed, a row's new pixels of alternating bytes and one entry: the colour at the run's start alone"""
    for w, rows in SIZES:
        shown, nxt = A.pair("index run", w, rows, half=half)
        if w > 1:
            assert (nxt[:, 1:] != nxt[:, :-1]).any(axis=2).all()
        text = host.emitter_delta256_rgb8(shown, nxt, half)
        if half:
            assert text.size == ((rows + 1) // 2) * (14 + 20 + 3 * w + 4)
            assert text.tobytes().count(b"\033[38;5;") == (rows + 1) // 2 and text.tobytes().count(b"48;5;") == (rows + 1) // 2
        else:
            assert text.size == rows * (14 + 11 + 2 * w + 4)
            assert text.tobytes().count(b"\033[48;5;") == rows


@pytest.mark.parametrize("half", [False, True], ids=HALF_IDS)
def test_the_longest_text_is_the_bound(half):
    """full cells: changed and unchanged cells in turn, 13 w + 13 + 5 ((w + 1) / 2) bytes a row -- more than one run of every cell, 13 w + 18;
    half-block cells: one run of every cell, 23 w + 18 a text row, but for an odd frame's last text row"""
    for w, rows in SIZES + [(4, 2), (64, 3), (65, 2)]:
        shown, nxt = A.pair("longest", w, rows, half=half)
        text = host.emitter_delta256_rgb8(shown, nxt, half)
        if half:
            assert text.size == A.bound(w, rows, True) - (9 * (w - 1) if rows % 2 else 0)
            assert hip_capacity(w, rows, True) == A.bound(w, rows, True)
        else:
            assert text.size == A.bound(w, rows) == hip_capacity(w, rows, False)
            assert text.size >= rows * (13 * w + 18)
    assert A.bound(1, 1) == 31 and A.bound(2, 1) == 44 and A.bound(1, 1, True) == 41


def hip_capacity(w, rows, half):
    """trt_ansi256_delta_capacity / trt_ansi256_delta_half_capacity: arithmetic on the host, no GPU"""
    return hip.ansi256_delta_capacity(w, rows, half)


def test_the_capacities():
    """the larger of the whole palette text and the bound; 0 at and beyond the limits and for sizes that are not positive"""
    for w, rows in SIZES + [(160, 48), (160, 47), (49999, 99999)]:
        assert hip_capacity(w, rows, False) == max(6 + (13 * w + 5) * rows, A.bound(w, rows))
    for w, rows in SIZES + [(160, 48), (160, 47), (99999, 199998), (99999, 199997)]:
        assert hip_capacity(w, rows, True) == max(6 + (23 * w + 5) * ((rows + 1) // 2), A.bound(w, rows, True))
    for w, rows in [(50000, 1), (1, 100000), (0, 1), (1, 0), (-1, 5), (5, -1)]:
        assert hip_capacity(w, rows, False) == 0, (w, rows)
    for w, rows in [(100000, 1), (1, 199999), (0, 1), (1, 0), (-1, 5), (5, -1)]:
        assert hip_capacity(w, rows, True) == 0, (w, rows)


@pytest.mark.parametrize("half", [False, True], ids=HALF_IDS)
def test_the_oracles_orbit(half):
    """consecutive frames of the demo orbit at 160 x 48 as the oracle renders them: the model shows every frame, the palette delta's cells are a
    subset of the 24-bit delta's, and it is the shorter text"""
    frames = [D.oracle_rgb("demo", "synth", D.W, D.HEIGHT, k, D.B, D.SPP) for k in range(5)]
    for k in range(1, len(frames)):
        text = check_pair(frames[k - 1], frames[k], half, f"orbit frame {k}")
        other = host.emitter_delta_half_rgb8(frames[k - 1], frames[k]) if half else host.emitter_delta_rgb8(frames[k - 1], frames[k])
        assert 0 < text.size < other.size
