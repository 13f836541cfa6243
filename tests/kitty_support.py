"""What the tests of the kitty graphics-protocol image share (csrc/trt_kitty.h): a formatter written from the format's description with the
standard library's base64 as the independent encoder, and a STRUCTURAL READER, which stands in for the terminal nobody here has: it takes a
text apart into the home prefix and APC sequences, checks the keys and the chunking, and decodes the joined payload back to the frame."""
import base64
import re

import numpy as np

HOME = b"\033[0;0H"
CHUNK_PIXELS = 1024
FIRST_KEYS = {"a": "T", "f": "24", "i": "1", "p": "1", "q": "2", "C": "1"}  # and s, v, m


def length(w, h):
    return 4 * w * h + 10 * ((w * h + CHUNK_PIXELS - 1) // CHUNK_PIXELS) + 46


def formatter(rgb):
    """the format as its description states it: the home prefix, then the pixels' base64 cut into chunks of 1024 pixels, the first behind the
    48-byte header, the others behind 'm' alone, each ended by ESC backslash; m is 1 but in the last chunk"""
    rows, width, _ = rgb.shape
    flat = np.ascontiguousarray(rgb, dtype=np.uint8).reshape(-1, 3)
    chunks = [flat[i:i + CHUNK_PIXELS] for i in range(0, len(flat), CHUNK_PIXELS)]
    text = HOME
    for c, pixels in enumerate(chunks):
        more = 0 if c == len(chunks) - 1 else 1
        text += (b"\033_Ga=T,f=24,i=1,p=1,q=2,C=1,s=%05d,v=%05d,m=%d;" % (width, rows, more)) if c == 0 else (b"\033_Gm=0%d;" % more)
        text += base64.b64encode(pixels.tobytes()) + b"\033\\"
    return text


def every_value_image():
    i = np.arange(256)
    image = np.stack([i, 255 - i, (7 * i) & 255], axis=1).astype(np.uint8).reshape(16, 16, 3)
    assert all(len(set(image[..., ch].ravel())) == 256 for ch in range(3))
    return image


def read(text):
    """the structural reader: uint8 [rows, width, 3] of a text, every rule of the format asserted on the way"""
    text = bytes(text)
    assert text.startswith(HOME), text[:8]
    body = text[len(HOME):]
    assert b"\n" not in text and b"\0" not in text
    sequences = re.findall(rb"\033_G([^;\033]*);([^\033]*)\033\\", body)
    assert sequences and sum(len(keys) + len(payload) + 6 for keys, payload in sequences) == len(body), "bytes between or behind the APC sequences"
    payloads = []
    for c, (keys, payload) in enumerate(sequences):
        pairs = [item.split("=") for item in keys.decode("ascii").split(",")]
        assert all(len(pair) == 2 for pair in pairs) and len({k for k, _ in pairs}) == len(pairs), keys
        d = dict(pairs)
        if c == 0:
            assert set(d) == set(FIRST_KEYS) | {"s", "v", "m"} and all(d[k] == v for k, v in FIRST_KEYS.items()), keys
            assert len(keys) + 4 == 48 and len(d["s"]) == 5 and len(d["v"]) == 5 and d["s"].isdigit() and d["v"].isdigit(), keys
            width, rows = int(d["s"]), int(d["v"])
        else:
            assert set(d) == {"m"}, keys
        assert d["m"].isdigit() and int(d["m"]) == (0 if c == len(sequences) - 1 else 1), (c, keys)
        assert 0 < len(payload) <= 4 * CHUNK_PIXELS and len(payload) % 4 == 0, (c, len(payload))
        assert c == len(sequences) - 1 or len(payload) == 4 * CHUNK_PIXELS, (c, len(payload))
        assert re.fullmatch(rb"[A-Za-z0-9+/]*", payload), c
        payloads.append(payload)
    raw = base64.b64decode(b"".join(payloads), validate=True)
    assert len(raw) == 3 * width * rows and len(sequences) == (width * rows + CHUNK_PIXELS - 1) // CHUNK_PIXELS and len(text) == length(width, rows)
    return np.frombuffer(raw, dtype=np.uint8).reshape(rows, width, 3)
