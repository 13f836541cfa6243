"""Both whole terminal texts on the device at the widths either side of the switch in the shared position map (csrc/trt_text_map.h):
trt_text_advance finds a word's row by a compare where a row is at least as long as a wave's span, and by a multiply-high where it is
shorter.  The full text's rows are 25 w + 1 bytes against a span of 1536 (w = 61: 1526, w = 62: 1551), the half-block text's 39 w + 5
against 2304 (w = 58: 2267, w = 59: 2306).  One table for both kinds; the expected bytes are the host emitter's text of the oracle's
frame, and every byte outside the text is held against its guard value."""
import functools

import numpy as np
import pytest

import support as T
from terminalraytracer_amd import hip
from test_ansi_half_text import STORE, DeviceBytes, anim_cameras, full_text, half_text, same_text, scene

pytestmark = pytest.mark.gpu

# kind: (cell bytes, end bytes, words a wave stores, the host emitter's text, the text's length, the device entry, the formatting alone)
KINDS = {
    "full": (25, 1, 384, full_text, hip.ansi_bytes, "render_device_ansi", "ansi_from_rgb8"),
    "half": (39, 5, hip.ANSI_HALF_WAVE_WORDS, half_text, hip.ansi_half_bytes, "render_device_ansi_half", "ansi_half_from_rgb8"),
}
# (kind, width, rows): the widths either side of the switch; an odd frame, and for the half-block text an even one too
SCREENS = [("full", 61, 3), ("full", 62, 3), ("half", 58, 3), ("half", 58, 4), ("half", 59, 3), ("half", 59, 4)]
CASES = [(kind, w, h, spp) for kind, w, h in SCREENS for spp in (1, 3)]
IDS = [f"{kind}_{w}x{h}_spp{spp}" for kind, w, h, spp in CASES]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.set_scene(scene("demo"))
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def oracle(kind, w, h, spp):
    """(the oracle's frame as the emitter's bytes, the host emitter's text of them) -- computed once, never written to"""
    px, _ = T.oracle_render(scene("demo").with_camera(anim_cameras([7], w, h)[0]), w, h, 4, spp)
    rgb = T.oracle_rgb8(px)
    text = KINDS[kind][3](rgb)
    rgb.flags.writeable = text.flags.writeable = False
    return rgb, text


def test_the_widths_lie_either_side_of_each_kinds_switch():
    for kind, (cell, end, wave_words, *_) in KINDS.items():
        below, above = sorted({w for k, w, _ in SCREENS if k == kind})
        assert above == below + 1 and cell * below + end < STORE * wave_words <= cell * above + end


@pytest.mark.parametrize("kind,w,h,spp", CASES, ids=IDS)
def test_the_device_entry_either_side_of_the_switch_at_every_alignment(ctx, kind, w, h, spp):
    _, _, _, _, length, entry, _ = KINDS[kind]
    want = oracle(kind, w, h, spp)[1]
    n = length(w, h)
    assert n == want.size
    for offset in range(STORE):
        mem = DeviceBytes(n, offset)
        getattr(ctx, entry)(anim_cameras([7], w, h)[0], hip.RowSet.whole(w, h), 4, spp, mem.ptr, n)
        same_text(mem.read(ctx, f"offset {offset}"), want, f"{kind} {w}x{h} spp {spp} at offset {offset}")


@pytest.mark.parametrize("kind,w,h,spp", CASES, ids=IDS)
def test_the_formatting_alone_either_side_of_the_switch_at_every_alignment(ctx, kind, w, h, spp):
    import torch
    _, _, _, _, length, _, formatting = KINDS[kind]
    rgb, want = oracle(kind, w, h, spp)
    src = torch.from_numpy(rgb.reshape(-1).copy()).to("cuda:0")
    torch.cuda.synchronize()
    for offset in range(STORE):
        mem = DeviceBytes(length(w, h), offset)
        getattr(ctx, formatting)(src.data_ptr(), w, h, mem.ptr)
        same_text(mem.read(ctx, f"offset {offset}"), want, f"{kind} {w}x{h} spp {spp} from bytes at offset {offset}")
