"""Constructed pairs of oriented boxes on the branches of the Sutherland-Hodgman clip (clipping.rs:12-91): collinear and almost
parallel edges, vertices on an edge line, concentric boxes, slivers far from the origin.  On these the reference itself returns NaN,
IoU above 1 or rounding noise, so "bit for bit" holds only if every inside test and every 1 / 0 of a clipper comes out as the
reference's.  Plain helper module (no fixtures): the CPU tests (tests/test_device_logic_emu.py) and the GPU tests
(tests/test_gpu_degenerate_boxes.py) share it.

A box is (xc, yc, angle | None, aspect, height), every number rounded to f32 before anything is derived from it.  For a base box
partners() yields (family, box):

  same centre    same           the base itself
                 angle:<d>      angle + d, d in pi/2, pi, +-1e-7, 1e-4, pi/2 + 1e-7 (1e-7 is at least one f32 ulp of the angle)
                 height:<f>     height x 0.5, 2, 1 + 1e-6 (nested)
                 aspect:<f>     aspect x f at the same angle: two edges collinear, the family with NaN intersections
                 aspect:inv     aspect 1 / a
                 no_angle       no angle at all, against a base of angle 0.0 only
  shifted        shift:<dir>:<k>:<d>   by k widths along the base's own x axis (dir x), k heights along its own y axis (dir y), or both
                 (dir c: corner to corner); k in 0.5, 1, 1 +- 1e-9, 1 +- 1e-7, 1 +- 1e-5, 1 +- 1e-3; partner angle + d, d in 0, pi/2,
                 pi, +-1e-7, 1e-4
                 other:<dir>:<k>:<d>   a partner of another aspect and height placed the same way: by k x the mean of the two boxes'
                 extents along that axis, so that k = 1 touches (at d = pi/2 the partner's extents swap)
  ulp            ulp:<axis><sign>      the centre moved by one f32 ulp

pairs() returns every pair in both orders."""
import functools
import math

import numpy as np

from similari_amd import abi

f32 = np.float32
PI = math.pi
MAGS = (0.0, 10.0, 1e3, 1e5, 1e6)
THETAS = (0.0, 1e-9, 1e-7, 1e-4, 0.3, PI / 4, PI / 2, PI, -PI, 2 * PI, 7.0, -3.0)
KS = (0.5, 1.0, 1 - 1e-9, 1 + 1e-9, 1 - 1e-7, 1 + 1e-7, 1 - 1e-5, 1 + 1e-5, 1 - 1e-3, 1 + 1e-3)
SAME_CENTRE_ANGLES = (PI / 2, PI, 1e-7, -1e-7, 1e-4, PI / 2 + 1e-7)
SHIFT_ANGLES = (0.0, PI / 2, PI, 1e-7, -1e-7, 1e-4)
ASPECT_FACTORS = (0.6824718, 1.5, 0.999999)

# truly disjoint slivers (gap ~0.005) at coordinates of 1e6 whose long edges are one f32 ulp of the angle from parallel: with the first as
# the subject the reference's clip returns 0.9655, IoU 0.558 (the emptiness proof of the positional tiles used to drop this pair), the
# other way round 0.0
EXAMPLE_PAIR = ((1000000.0, 1000000.06, 1.5707963, 0.00229841, 24.218212), (1000000.0, 1000000.0, 1.5707964, 0.00229841, 24.218212))
# concentric boxes smaller than the f32 spacing of their coordinates, turned by 1e-7 .. 1e-2 rad or a hair different in height (the
# angle and height families above, found by drawing ~1e7 of them): the reference's clip result has 12 vertices, which is SA_POLY_CAP,
# the length of the lane-parallel clippers' vertex lists — or 13, which overflows them in the last pass (the pair then goes to the
# serial clipper, whose lists cannot overflow).  For the second of the 13s the reference's IoU is -1.43; lists cut at 12 gave 21.88.
TWELVE_VERTEX_PAIRS = (
    ((1000000.0, 1000300.0, 0.598061502, 0.00552795455, 0.0130355107), (1000000.0, 1000300.0, 0.598061383, 0.00552795455, 0.0130354976)),
    ((1000000.0, 1000600.0, -6.44522047, 0.0021096, 0.0208491385), (1000000.0, 1000600.0, -6.44522047, 0.0021096, 0.020849118)),
    ((1000000.0, 1000900.0, 0.250813425, 0.0445149429, 0.0233292058), (1000000.0, 1000900.0, 0.250813335, 0.0445149429, 0.0233292058)),
)
THIRTEEN_VERTEX_PAIRS = (
    ((1000000.0, 1001200.0, -1.28735399, 0.0716044307, 0.0151240081), (1000000.0, 1001200.0, -1.28735411, 0.0716044307, 0.015124023)),
    ((1000000.0, 1000000.0, 7.000999927520752, 0.2880050837993622, 0.012967241927981377),
     (1000000.0, 1000000.0, 7.0, 0.2880050837993622, 0.012967228889465332)),
    ((1000000.0, 1001500.0, 2.31063485, 0.00348166702, 0.0600201003), (1000000.0, 1001500.0, 2.31073475, 0.00348166702, 0.0600200407)),
    ((1000000.0, 1001800.0, 6.38154173, 0.00425084727, 0.11431434), (1000000.0, 1001800.0, 6.38154173, 0.00425084727, 0.114314355)),
)


def r32(x):
    return float(f32(x))


def turned(theta, d):
    """f32(theta + d), at least one ulp away from theta in d's direction."""
    t = f32(theta + d)
    if d != 0.0 and t == f32(theta):
        t = np.nextafter(f32(theta), f32(math.copysign(math.inf, d)))
    return float(t)


def partners(xc, yc, a, h, theta, other=(0.37, 2.3)):
    """(family, box) for every partner of the base box (xc, yc, theta, a, h); other = (aspect factor, height factor) of the `other:` family."""
    xc, yc, a, h, theta = r32(xc), r32(yc), r32(a), r32(h), r32(theta)
    w = a * h
    c, s = math.cos(theta), math.sin(theta)
    out = [("same", (xc, yc, theta, a, h))]
    for d in SAME_CENTRE_ANGLES:
        out.append((f"angle:{d:.8g}", (xc, yc, turned(theta, d), a, h)))
    for f in (0.5, 2.0, 1 + 1e-6):
        out.append((f"height:{f:.8g}", (xc, yc, theta, a, r32(h * f))))
    for f in ASPECT_FACTORS:
        out.append((f"aspect:{f:.8g}", (xc, yc, theta, r32(a * f), h)))
    out.append(("aspect:inv", (xc, yc, theta, r32(1.0 / a), h)))
    if theta == 0.0:
        out.append(("no_angle", (xc, yc, None, a, h)))
    a2, h2 = r32(a * other[0]), r32(h * other[1])
    for fam, pa, ph in (("shift", a, h), ("other", a2, h2)):
        pw = pa * ph
        for d in SHIFT_ANGLES:
            swap = fam == "other" and d == PI / 2      # the partner's extents along the base's axes
            ex, ey = (ph, pw) if swap else (pw, ph)
            sx, sy = (w + ex) / 2, (h + ey) / 2        # fam "shift": the base's own width and height
            for k in KS:
                for direction, fx, fy in (("x", 1.0, 0.0), ("y", 0.0, 1.0), ("c", 1.0, 1.0)):
                    dx = k * (fx * sx * c - fy * sy * s)
                    dy = k * (fx * sx * s + fy * sy * c)
                    out.append((f"{fam}:{direction}:{k:.10g}:{d:.8g}", (r32(xc + dx), r32(yc + dy), turned(theta, d), pa, ph)))
    inf = f32(math.inf)
    for axis, v in (("x", xc), ("y", yc)):
        for sign, to in (("+", inf), ("-", -inf)):
            m = float(np.nextafter(f32(v), to))
            out.append((f"ulp:{axis}{sign}", (m if axis == "x" else xc, m if axis == "y" else yc, theta, a, h)))
    return out


def bases(seed=20250, random_thetas=22, mags=MAGS, max_radius=None):
    """(mag, a, h, theta) of the base boxes: per magnitude the fixed angles and `random_thetas` uniform draws in [-7, 7], each with an
    aspect log-uniform in [1e-3, 1e3] and a height log-uniform in [1e-2, 1e3] (max_radius: redrawn until the half diagonal fits)."""
    rng = np.random.default_rng(seed)
    out = []
    for mag in mags:
        for theta in list(THETAS) + list(rng.uniform(-7.0, 7.0, random_thetas)):
            while True:
                a = float(np.exp(rng.uniform(math.log(1e-3), math.log(1e3))))
                h = float(np.exp(rng.uniform(math.log(1e-2), math.log(1e3))))
                if max_radius is None or 0.5 * h * math.hypot(1.0, a) <= max_radius:
                    break
            out.append((mag, r32(a), r32(h), r32(theta)))
    return out


def to_boxes(rows, confidence=1.0):
    """sa_box array of box tuples (angle None = no angle)."""
    b = abi.make_boxes([r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows], [r[4] for r in rows],
                       confidence=np.full(len(rows), confidence, np.float32))
    for i, r in enumerate(rows):
        if r[2] is not None:
            b["has_angle"][i], b["angle"][i] = 1, r[2]
    return b


@functools.lru_cache(maxsize=None)
def pairs(seed=20250, random_thetas=22):
    """Every pair of every base at xc = yc = mag, in both orders, plus EXAMPLE_PAIR and the 12- and 13-vertex pairs (subject first).  Returns
    (A, B, family): two sa_box arrays and a list of family names; rows 2k and 2k + 1 are one pair in its two orders.  The arrays are
    shared and read-only."""
    rng = np.random.default_rng(seed + 1)
    ra, rb, fam = [], [], []
    for mag, a, h, theta in bases(seed, random_thetas):
        other = (float(np.exp(rng.uniform(math.log(0.25), math.log(4.0)))), float(np.exp(rng.uniform(math.log(0.25), math.log(4.0)))))
        base = (r32(mag), r32(mag), theta, a, h)
        for name, box in partners(mag, mag, a, h, theta, other):
            ra += [base, box]
            rb += [box, base]
            fam += [name, name]
    for name, (p, q) in [("example", EXAMPLE_PAIR)] + [("twelve", pq) for pq in TWELVE_VERTEX_PAIRS] + [("thirteen", pq) for pq in THIRTEEN_VERTEX_PAIRS]:
        ra += [p, q]
        rb += [q, p]
        fam += [name, name]
    A, B = to_boxes(ra), to_boxes(rb)
    A.flags.writeable = B.flags.writeable = False
    return A, B, fam


def touching(family):
    """The families whose boxes are placed edge to edge or corner to corner (and the example pair, which is such a placement)."""
    return family.startswith(("shift:", "other:")) or family == "example"


# ---- scenes: the same pairs, one per place, for whole frames ----------------------------------------------------------------------
def radius(box):
    return 0.5 * box[4] * math.hypot(1.0, box[3])


@functools.lru_cache(maxsize=None)
def placed_pairs(n, seed=20251, max_reach=100.0, lead="example"):
    """n pairs (track box, detection box), each at a place of its own: rows of pairs along x at y = mag, spaced by their reach (the
    distance from the base's centre to the far side of either bounding circle), so that a box is within too_far reach (bbox.rs:452-462)
    of its partner only.  Family after family in turn over bases of at most max_reach / 4 half diagonal, so that every family — the NaN
    family, identical boxes, every touching placement — is there about equally often; odd pairs are swapped (the track gets the partner);
    EXAMPLE_PAIR and the 12- and 13-vertex pairs (the detection is the subject) stand at their own coordinates, off the rows.  Returns (track
    rows, detection rows, families)."""
    rng = np.random.default_rng(seed)
    bs = bases(seed, random_thetas=12, max_radius=max_reach / 4)
    names = [name for name, _ in partners(0.0, 0.0, 1.0, 1.0, 0.0)]           # angle 0.0: every family exists
    start = {0.0: (0.0, -1.0), 10.0: (10.0 + 3 * max_reach, 1.0)}             # the rows of 0 and 10 leave the origin in opposite directions
    cursor = {}
    # (lead = "thirteen": the 13-vertex pair that stands where the example does takes its place — the one whose cell shows a lost vertex)
    lead_pair = EXAMPLE_PAIR if lead == "example" else next(pq for pq in THIRTEEN_VERTEX_PAIRS if pq[0][:2] == EXAMPLE_PAIR[1][:2])
    tr, dt, fam = [lead_pair[1]], [lead_pair[0]], [lead]
    for name, pq in [("twelve", pq) for pq in TWELVE_VERTEX_PAIRS] + [("thirteen", pq) for pq in THIRTEEN_VERTEX_PAIRS]:
        if pq[0][:2] == EXAMPLE_PAIR[1][:2]:                                  # (stands where the example does: see lead)
            continue
        tr.append(pq[1])
        dt.append(pq[0])
        fam.append(name)
    order = rng.permutation(len(names))
    k = 0
    while len(tr) < n:
        mag, a, h, theta = bs[int(rng.integers(len(bs)))]
        want = names[order[k % len(names)]]
        k += 1
        other = (float(np.exp(rng.uniform(math.log(0.25), math.log(4.0)))), float(np.exp(rng.uniform(math.log(0.25), math.log(4.0)))))
        local = dict(partners(0.0, 0.0, a, h, theta, other))
        if want not in local:                                                 # no_angle away from angle 0.0
            continue
        p = local[want]
        reach = max(radius((0, 0, theta, a, h)), math.hypot(p[0], p[1]) + radius(p))
        if reach > max_reach:
            continue
        x0, direction = start.get(mag, (mag + 2 * max_reach, 1.0))
        x, last = cursor.get(mag, (x0, 0.0))
        if last:
            x += direction * (last + reach + 1.0 + 1e-6 * abs(x))
        cursor[mag] = (x, reach)
        base = (r32(x), r32(mag), theta, a, h)
        box = dict(partners(x, mag, a, h, theta, other))[want]
        swap = k % 2 == 1
        tr.append(box if swap else base)
        dt.append(base if swap else box)
        fam.append(want)
    return tuple(tr), tuple(dt), tuple(fam)
