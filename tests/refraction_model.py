"""An exact model of ONE step of a path through the refraction extension (trt_set_refraction), in 60-digit decimal arithmetic.

The oracle's restatement of the extension (oracle/trt_oracle.c, shade_pixel_refractive) was written from the kernel, operation for
operation; a mistake the two share shows in no comparison of the two.  This model is written from the DECLARED rules instead (the
comment above trt_set_refraction in include/trt_hip.h) and from the textbook form of Snell's law -- split the direction into its normal
and tangential parts, scale the tangential part, rebuild the normal part -- not from the kernel's expressions.

It is fed the path rays the restatement logs for a frame.  For ray k of a sample it takes the LOGGED doubles (o_k, d_k) as exact inputs,
so that nothing accumulates along a path, and predicts (o_k+1, d_k+1), the state `inside` -- which is the model's own, from -1 at the eye
-- and, from the bounce and weight bookkeeping in float64, how many path rays the sample logs.

Which surface is the nearest is decided in float64 with numpy (for all rays at once), the chosen surface is then intersected in
decimal.  Where float64 cannot decide, the model declines the event and stops checking that sample:
  - the two nearest surfaces lie within 1e-7 of one another, relative to t;
  - the chosen sphere's disc / b^2 is below 1e-6 (a grazing hit: sqrt(disc) has lost its digits), or a sphere whose |disc| / b^2 is below
    1e-6 passes the ray no farther away than the chosen surface (hit or miss is then a matter of the last bit);
  - |1 - s2| < 1e-6 at a refractor (bend or total reflection is a matter of the last bits).
Only the standard library and numpy are used."""
import decimal
from decimal import Decimal

import numpy as np

PRECISION = 60
NUDGE = Decimal(0.000001)  # TRT.c:44 EPSILON, the double
SHORT = Decimal(0.0001)    # TRT.c:444: normalize_vector leaves a vector no longer than this alone
CLASSES = ("enter", "enter while inside another", "leave", "total reflection inside", "total reflection from outside", "ground while inside",
           "opaque sphere while inside", "ordinary hit")
MISTAKES = ("eta inverted", "normal not flipped on leaving", "refracted origin at p + back", "near root inside", "outer refractor remembered")
TIE, GRAZE, CRITICAL = 1e-7, 1e-6, 1e-6
ZERO, ONE, TWO = Decimal(0), Decimal(1), Decimal(2)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def _scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _unit(a):
    n = _dot(a, a).sqrt()
    return _scale(a, ONE / n) if n > SHORT else a


def _vec(row):
    return (Decimal(float(row[0])), Decimal(float(row[1])), Decimal(float(row[2])))


def split_samples(origins, eye):
    """[start, ...] + [len]: a sample starts where a path ray's origin is the eye, bit for bit"""
    o = np.ascontiguousarray(origins, dtype=np.float64).view(np.uint64).reshape(-1, 3)
    e = np.ascontiguousarray(eye, dtype=np.float64).view(np.uint64)
    return np.concatenate([np.nonzero((o == e).all(axis=1))[0], [len(o)]])


class Search:
    """the float64 part: every path ray of a frame against every sphere and the ground, at once"""

    def __init__(self, scene, rays):
        sph, g = scene.spheres, scene.ground
        o, d = rays[:, None, 0:3], rays[:, None, 3:6]
        with np.errstate(all="ignore"):
            oc = o - sph[None, :, 0:3]
            a = (d * d).sum(axis=2)
            b = 2.0 * (oc * d).sum(axis=2)
            c = (oc * oc).sum(axis=2) - sph[None, :, 3] ** 2
            disc = b * b - 4.0 * a * c
            root = np.sqrt(np.maximum(disc, 0.0))
            near, far = (-b - root) / (2.0 * a), (-b + root) / (2.0 * a)
            self.near = np.where((disc >= 0.0) & (near > 0.0), near, np.inf)
            self.far = np.where((disc >= 0.0) & (far > 0.0), far, np.inf)
            ratio = np.abs(disc) / (b * b)
            self.grazing = ~(ratio >= GRAZE)  # a NaN ratio (b == 0 and disc == 0) grazes
            self.closest = -b / (2.0 * a)      # where the ray passes the centre
            denom = rays[:, 3:6] @ g[3:6]
            t = ((g[0:3][None, :] - rays[:, 0:3]) @ g[3:6]) / denom
            self.ground = np.where((np.abs(denom) > 0.00001) & (t > 0.00001), t, np.inf)  # TRT.c:677-695

    def nearest(self, k, inside, near_root_inside=False):
        """(surface, declined): surface -2 the sky, -1 the ground, i a sphere"""
        t = self.near[k].copy()
        if inside >= 0 and not near_root_inside:
            t[inside] = self.far[k, inside]
        t = np.append(t, self.ground[k])
        order = np.argsort(t, kind="stable")
        best = t[order[0]]
        # a grazing sphere that is not the chosen one matters where it passes the ray before the chosen surface does: missed by a hair, it
        # would have been the nearest
        graze = bool((self.grazing[k] & (self.closest[k] > 0.0) & (self.closest[k] <= best * (1.0 + TIE))).any())
        if not np.isfinite(best):
            return -2, graze
        if t[order[1]] - best <= TIE * best:
            return -2, True
        which = int(order[0])
        if which == len(t) - 1:
            return -1, graze
        return which, graze or bool(self.grazing[k, which])


def _hit(o, d, scene_dec, which, far_root):
    """(hit point, unit normal) of ray (o, d) on surface `which`, in decimal"""
    centres, radii, gpoint, gnormal = scene_dec
    if which < 0:
        t = _dot(_sub(gpoint, o), gnormal) / _dot(d, gnormal)
        return _add(o, _scale(d, t)), _unit(gnormal)
    oc = _sub(o, centres[which])
    a, b, c = _dot(d, d), TWO * _dot(oc, d), _dot(oc, oc) - radii[which] * radii[which]
    root = (b * b - 4 * a * c).sqrt()
    t = (-b + root if far_root else -b - root) / (TWO * a)
    p = _add(o, _scale(d, t))
    return p, _unit(_sub(p, centres[which]))


def _bend(d, nn, eta, check):
    """Snell's law about the facing unit normal nn: (new direction or None at the critical angle, totally reflected?)"""
    d_n = _scale(nn, _dot(d, nn))
    d_t = _sub(d, d_n)
    s2 = eta * eta * _dot(d_t, d_t)
    if abs(ONE - s2) < Decimal(CRITICAL):
        return None, False
    if s2 > ONE:
        out = _unit(_sub(d, _scale(d_n, TWO)))
        if check:
            assert _dot(out, nn) > 0, "a totally reflected ray stays on its side"
        return out, True
    out = _unit(_sub(_scale(d_t, eta), _scale(nn, (ONE - s2).sqrt())))
    if check:  # the model's own output: Snell's ratio, the plane of incidence, the side
        tiny = Decimal(10) ** -50
        assert abs(_dot(_cross(out, nn), _cross(out, nn)).sqrt() - eta * _dot(_cross(d, nn), _cross(d, nn)).sqrt()) < tiny
        assert abs(_dot(out, _cross(d, nn))) < tiny
        assert _dot(out, nn) < 0, "a refracted ray goes through the surface"
    return out, False


def check_frame(scene, ior, rays, bounce_limit, tolerance=1e-10, mistake=None, stop_after=None):
    """Judge the logged path rays (float64 [n, 6], in trace order) of one single-threaded frame of the restatement.

    Returns {"samples", "events", "declined", "classes": {class: judged events}, "origin", "direction": the largest deviations of a judged
    event, "worst": where they were, "wrong rays": judged events beyond the tolerance, "wrong lengths": samples that log another number of
    path rays than predicted, "first": a description of the first disagreement}.  `mistake`: one of MISTAKES, planted into the model;
    `stop_after`: give up after that many disagreements."""
    assert mistake is None or mistake in MISTAKES
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    ior = np.asarray(ior, dtype=np.float64)
    search = Search(scene, rays)
    starts = split_samples(rays[:, 0:3], scene.camera[9:12])
    assert len(starts) > 1 and starts[0] == 0
    out = {"samples": len(starts) - 1, "events": 0, "declined": 0, "classes": dict.fromkeys(CLASSES, 0), "origin": 0.0, "direction": 0.0,
           "worst": {}, "wrong rays": 0, "wrong lengths": 0, "first": None}
    refl = scene.spheres[:, 7]
    g_even, g_odd = float(scene.ground[9]), float(scene.ground[14])

    def wrong(kind, what):
        out[kind] += 1
        if out["first"] is None:
            out["first"] = what

    with decimal.localcontext() as ctx:
        ctx.prec = PRECISION
        scene_dec = ([_vec(s[0:3]) for s in scene.spheres], [Decimal(float(s[3])) for s in scene.spheres], _vec(scene.ground[0:3]), _vec(scene.ground[3:6]))
        ior_dec = [Decimal(float(v)) if v > 0.0 else None for v in ior]
        tol = Decimal(tolerance)
        for s in range(len(starts) - 1):
            if stop_after is not None and out["wrong rays"] + out["wrong lengths"] >= stop_after:
                break
            k, end = int(starts[s]), int(starts[s + 1])
            inside, outer, bounces, weight = -1, [], 0, 1.0
            while True:
                out["events"] += 1
                which, declined = search.nearest(k, inside, mistake == "near root inside")
                if declined:
                    out["declined"] += 1
                    break
                if which == -2:  # the sky ends the sample
                    if end != k + 1:
                        wrong("wrong lengths", f"sample {s}: the model meets the sky at ray {k - int(starts[s])}, the log goes on")
                    break
                o, d = _vec(rays[k, 0:3]), _vec(rays[k, 3:6])
                leaving = which >= 0 and which == inside
                p, n = _hit(o, d, scene_dec, which, leaving and mistake != "near root inside")
                back = _scale(_unit(_sub(o, p)), NUDGE)
                bends = which >= 0 and ior_dec[which] is not None
                if bends:
                    nn = n if (not leaving or mistake == "normal not flipped on leaving") else _scale(n, -ONE)
                    eta = ior_dec[which] if leaving else ONE / ior_dec[which]
                    if mistake == "eta inverted":
                        eta = ONE / eta
                    new_d, mirrored = _bend(d, nn, eta, mistake is None)
                    if new_d is None:
                        out["declined"] += 1
                        break
                    if mirrored:
                        new_o, kind = _add(p, back), "total reflection inside" if leaving else "total reflection from outside"
                    else:
                        new_o = _add(p, back) if mistake == "refracted origin at p + back" else _sub(p, back)
                        kind = "leave" if leaving else ("enter" if inside < 0 else "enter while inside another")
                        if mistake == "outer refractor remembered":
                            if leaving:
                                inside = outer.pop() if outer else -1
                            else:
                                if inside >= 0:
                                    outer.append(inside)
                                inside = which
                        else:
                            inside = -1 if leaving else which
                else:
                    new_d, new_o = _unit(_sub(d, _scale(n, TWO * _dot(d, n)))), _add(p, back)
                    kind = "ordinary hit" if inside < 0 else ("ground while inside" if which < 0 else "opaque sphere while inside")
                # the bookkeeping, in float64 and in the restatement's order
                if not leaving:
                    if which >= 0:
                        weight *= float(refl[which])
                    else:
                        hit = rays[k, 0:3] + search.ground[k] * rays[k, 3:6]
                        weight *= g_odd if (int(np.floor(hit[0]) + np.floor(hit[2])) & 1) else g_even
                bounces += 1
                if not (bounces < bounce_limit and weight > 0.00001):
                    if end != k + 1:
                        wrong("wrong lengths", f"sample {s}: the model ends the path after ray {k - int(starts[s])}, the log goes on")
                    break
                if end == k + 1:
                    wrong("wrong lengths", f"sample {s}: the log ends after ray {k - int(starts[s])}, the model goes on ({kind})")
                    break
                dev_o = float(max(abs(a - b) for a, b in zip(new_o, _vec(rays[k + 1, 0:3]))))
                dev_d = float(max(abs(a - b) for a, b in zip(new_d, _vec(rays[k + 1, 3:6]))))
                if not (dev_o <= tol and dev_d <= tol):
                    wrong("wrong rays", f"sample {s}, ray {k - int(starts[s])}, {kind} at surface {which}: origin off by {dev_o:.3g}, direction by {dev_d:.3g}")
                    break
                out["classes"][kind] += 1
                for name, dev in (("origin", dev_o), ("direction", dev_d)):
                    if dev > out[name]:
                        out[name], out["worst"][name] = dev, (s, k - int(starts[s]), kind, which)
                k += 1
    return out
