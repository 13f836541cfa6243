"""ONE filtered sky look-up, written from the declared rules above trt_set_sky_filter in include/trt_hip.h -- not from the kernels and
not from tests/sky_filter_restatement.c.

Every operation is a correctly rounded binary64 multiplication, addition, division or square root, or the reference's normalisation:
those of tests/exact_ieee.py, which works on bit patterns with Python integers -- each result is the exact rational, rounded once --
and shares no floating-point unit with what it judges.  So the model predicts the face, the four taps, the two weights and the
colour bit for bit from the direction and the sky; nothing accumulates along a path.

    dir      = normalize_vector(direction)                        TRT.c:702
    f        = the first face whose axis has the largest dot product with dir, above -1          TRT.c:703-713
    u, v     = TRT.c:717-761 through the axis table, clamped to +-0.5                               TRT.c:778-779
    x        = clamp((u + 0.5) * dim - 0.5, 0, dim - 1);   i0 = (int)x;  fx = x - i0;  i1 = min(i0 + 1, dim - 1);   y, j0, fy, j1 from v
    c        = (top + (bot - top) * fy) / 255,  top = t00 + (t10 - t00) * fx,  bot = t01 + (t11 - t01) * fx,   per channel
    no face, or u or v not a number: face 0, four times texel 0, fx = fy = 0
"""
import exact_ieee as X

ZERO, ONE, HALF, MINUS_HALF, MINUS_ONE = (X.to_bits(v) for v in (0.0, 1.0, 0.5, -0.5, -1.0))
B255 = X.to_bits(255.0)
AXES = tuple(tuple(X.to_bits(c) for c in axis) for axis in
             ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)))  # TRT.c:137-143
BYTES = tuple(X.to_bits(float(b)) for b in range(256))


def dot(a, b):
    return X.add_bits(X.add_bits(X.mul_bits(a[0], b[0]), X.mul_bits(a[1], b[1])), X.mul_bits(a[2], b[2]))


def neg(a):
    return a ^ X.SIGN


def sub(a, b):
    return X.add_bits(a, neg(b))


def clamp(v, lo, hi):
    """the reference's: a NaN passes through"""
    if X.greater_bits(lo, v):
        return lo
    if X.greater_bits(v, hi):
        return hi
    return v


def truncated(x):
    """(int)x of a finite pattern 0 <= x < 2^31"""
    m, e = X.decode(x)
    return m << e if e >= 0 else m >> -e


def face_and_coordinates(direction):
    """(face or -1, u, v) of a direction given as three patterns; u, v clamped"""
    x, y, z, _ = X.unit_bits(*direction)
    d = [x, y, z]
    face, largest = -1, MINUS_ONE
    for f in range(6):
        along = dot(d, AXES[f])
        if X.greater_bits(along, largest):
            largest, face = along, f
    if face < 0:
        return face, X.NAN, X.NAN
    axis = AXES[face]
    touching = [X.mul_bits(c, a) for c, a in zip(d, axis)]
    by = X.div_bits(ONE, X.add_bits(X.add_bits(touching[0], touching[1]), touching[2]))
    d = [X.mul_bits(c, by) for c in d]
    along = dot(d, axis)
    flat = [X.mul_bits(sub(c, X.mul_bits(a, along)), HALF) for c, a in zip(d, axis)]
    u, v = dot(flat, AXES[(face + 2) % 6]), dot(flat, AXES[(face + 4) % 6])
    if face % 2 == 1:
        u = X.mul_bits(u, MINUS_ONE)
    if face < 2:
        u, v = v, neg(u)
    elif face < 4:
        u, v = neg(v), u
    elif face == 4:
        u, v = X.mul_bits(u, MINUS_ONE), X.mul_bits(v, MINUS_ONE)
    return face, clamp(u, MINUS_HALF, HALF), clamp(v, MINUS_HALF, HALF)


def taps_of(coordinate, dim):
    """(lower tap, upper tap, weight as a pattern) along one axis"""
    dim_f = X.to_bits(float(dim))
    scaled = X.mul_bits(X.add_bits(coordinate, HALF), dim_f)
    x = clamp(sub(scaled, HALF), ZERO, sub(dim_f, ONE))
    i0 = truncated(x)
    return i0, (i0 + 1 if i0 + 1 < dim else i0), sub(x, X.to_bits(float(i0)))


def lerp(a, b, f):
    return X.add_bits(a, X.mul_bits(sub(b, a), f))


def lookup(direction, sky):
    """direction: three patterns; sky: uint8[6, dim, dim, 3].  Returns {"face", "taps": (i0, j0, i1, j1), "fx", "fy" (patterns),
    "texels": four (r, g, b) in the order t00 t10 t01 t11, "colour": three patterns}"""
    dim = sky.shape[1]
    face, u, v = face_and_coordinates(direction)
    if face < 0 or X.is_nan(u) or X.is_nan(v):
        face, i0, i1, j0, j1, fx, fy = 0, 0, 0, 0, 0, ZERO, ZERO
    else:
        i0, i1, fx = taps_of(u, dim)
        j0, j1, fy = taps_of(v, dim)
    texels = [tuple(int(b) for b in sky[face, j, i]) for i, j in ((i0, j0), (i1, j0), (i0, j1), (i1, j1))]
    colour = []
    for c in range(3):
        t00, t10, t01, t11 = (BYTES[t[c]] for t in texels)
        top, bot = lerp(t00, t10, fx), lerp(t01, t11, fx)
        colour.append(X.div_bits(lerp(top, bot, fy), B255))
    return {"face": face, "taps": (i0, j0, i1, j1), "fx": fx, "fy": fy, "texels": texels, "colour": colour}
