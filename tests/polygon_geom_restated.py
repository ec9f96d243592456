"""Float64 numpy restatement of the minimum-area rectangle of a point set, the arbiter of the polygon-geometry tests (there is no
OpenCV here; the reference's cv2.minAreaRect works in float32 and resolves equal areas by its own traversal, so it could not arbitrate
at 1e-9 anyway).  It shares nothing with slenderobjdet_amd/structures/polygons.py except coco_gt._hull: one edge at a time, extents by
matrix products as coco_gt.min_area_rect_sides takes them, np.hypot for the edge length, the fold of the angle by repeated +-90 steps
as concern.support.rbox_from_polygon does it.

Also the seeded generator of annotations both test files use.
"""
import math

import numpy as np

from slenderobjdet_amd.evaluation.coco_gt import _hull

SEED = 20261019


def canonical(w, h, a):
    """(w, h, a) with a in (-45, 45]: quarter turns taken off the angle, w and h swapped at each."""
    while a > 45.0:
        a -= 90.0
        w, h = h, w
    while a <= -45.0:
        a += 90.0
        w, h = h, w
    return w, h, a + 0.0


def min_area_rect(points):
    """(rect (cx, cy, w, h, angle_deg), hull size, sorted [(area, direction in [0, 90))] over all hull edges) of [n, 2] points.
    Fewer than 3 hull vertices: the axis-aligned extent, angle 0, and an empty list."""
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    hull = _hull(pts)
    if len(hull) < 3:
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        return (float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2), float(hi[0] - lo[0]), float(hi[1] - lo[1]), 0.0), len(hull), []
    best, edges = None, []
    for i in range(len(hull)):
        e = hull[(i + 1) % len(hull)] - hull[i]
        u = e / np.hypot(e[0], e[1])
        v = np.array([-u[1], u[0]])
        pu, pv = hull @ u, hull @ v
        w, h = pu.max() - pu.min(), pv.max() - pv.min()
        a = math.degrees(math.atan2(-u[1], u[0]))
        edges.append((float(w * h), a % 90.0))
        if best is None or w * h < best[0]:      # the first minimal edge from the lexicographically smallest vertex
            c = u * (pu.min() + pu.max()) / 2 + v * (pv.min() + pv.max()) / 2
            best = (w * h, c, w, h, a)
    _, c, w, h, a = best
    w, h, a = canonical(w, h, a)
    return (float(c[0]), float(c[1]), float(w), float(h), float(a)), len(hull), sorted(edges)


def direction_gap(d0, d1):
    """Distance in degrees of two directions taken modulo 90."""
    d = abs(d0 - d1) % 90.0
    return min(d, 90.0 - d)


def is_tie(edges, rel=1e-9, apart=1e-6):
    """Does an edge of another direction (more than ``apart`` degrees away modulo 90) come within ``rel`` of the least area?"""
    if not edges:
        return False
    a0, d0 = edges[0]
    return any(a <= a0 * (1 + rel) and direction_gap(d, d0) > apart for a, d in edges[1:])


def encloses(rect, points, tol):
    """Do all points lie in the rectangle widened by ``tol`` on every side?  Width axis (cos a, -sin a), height axis (sin a, cos a)."""
    cx, cy, w, h, a = rect
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    t = math.radians(a)
    dx, dy = pts[:, 0] - cx, pts[:, 1] - cy
    pu = dx * math.cos(t) - dy * math.sin(t)
    pv = dx * math.sin(t) + dy * math.cos(t)
    return bool(np.all(np.abs(pu) <= w / 2 + tol) and np.all(np.abs(pv) <= h / 2 + tol))


def hull_has_near_collinear(points, rel=1e-9):
    """Does the oracle's hull hold three neighbouring vertices whose cross product is below rel * scale^2 (or fewer than three
    vertices)?  Another correct hull may then count one vertex more or less."""
    pts = np.asarray(points, np.float64).reshape(-1, 2)
    hull = _hull(pts)
    if len(hull) < 3:
        return True
    scale = max(1.0, float(np.abs(pts).max()))
    a, b = np.roll(hull, -1, axis=0) - hull, np.roll(hull, -2, axis=0) - hull
    return bool((np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]) < rel * scale * scale).any())


def _rotate(p, deg, about):
    t = math.radians(deg)
    c, s = math.cos(t), math.sin(t)
    d = p - about
    return about + np.stack([d[:, 0] * c - d[:, 1] * s, d[:, 0] * s + d[:, 1] * c], axis=1)


# integer direction vectors of integer length: a rectangle along one has corners on the 0.01 grid, so rounding leaves it exact
_TRIPLES = ((1, 0, 1), (3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29))


def generate(count, seed=SEED):
    """``count`` annotations as lists of polygons (flat coordinate lists, rounded to 2 decimals as COCO's are).  Per annotation
    n = randint(3, 200) points in one of three layouts: uniform in a box; the same squeezed along one axis to 0.02-0.2 and turned by a
    random angle ("slender"); an exact turned rectangle or (7 in 100, and whenever n = 3) a triangle, with the other points inside.
    One annotation in three with at least 9 points is split into 2-3 polygons.

    The rectangles lie along Pythagorean directions, so that their corners are on the 0.01 grid and the rounding leaves them
    rectangles: a rectangle turned by an arbitrary angle becomes a general quadrilateral, and wherever the two angles at an edge and
    the two at its neighbour are all at most 90 degrees both edges give twice the area of one triangle - an exact tie of two
    directions ~0.005 / side apart, which the parity tests would have to exclude.  Every acute triangle is a three-way tie."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        n = int(rs.randint(3, 201))
        layout = int(rs.randint(3))
        if layout < 2:
            p = rs.rand(n, 2) * (640, 480) * rs.rand() + rs.rand(2) * 100
            if layout == 1:
                axis = int(rs.randint(2))
                mid = p.mean(axis=0)
                p[:, axis] = mid[axis] + (p[:, axis] - mid[axis]) * rs.uniform(0.02, 0.2)
                p = _rotate(p, rs.uniform(0, 360), mid)
        else:
            if rs.rand() < 0.93 and n >= 4:
                a, b, c = _TRIPLES[rs.randint(len(_TRIPLES))]
                if rs.rand() < 0.5:
                    a, b = b, a
                a, b = a * rs.choice((-1, 1)), b * rs.choice((-1, 1))
                ws, hs = np.round(rs.uniform(4, 400, 2) / c, 2)                    # W = c * ws, H = c * hs
                start = np.round(rs.rand(2) * (640, 480), 2)
                corners = start + np.array([[0, 0], [a * ws, b * ws], [a * ws - b * hs, b * ws + a * hs], [-b * hs, a * hs]])
                t = 0.05 + 0.9 * rs.rand(n - 4, 2)
                inner = start + t[:, :1] * np.array([a * ws, b * ws]) + t[:, 1:] * np.array([-b * hs, a * hs])
                p = np.concatenate([corners, inner])
            else:
                tri = rs.rand(3, 2) * (640, 480)
                bary = rs.dirichlet((1, 1, 1), n - 3)
                inner = tri.mean(axis=0) + (bary @ tri - tri.mean(axis=0)) * 0.9
                p = np.concatenate([tri, inner])
            p = p[rs.permutation(len(p))]
        p = np.round(p, 2)
        parts = int(rs.randint(2, 4)) if (n >= 9 and rs.rand() < 1 / 3) else 1
        extra = np.sort(rs.randint(0, n - 3 * parts + 1, parts - 1))                 # every part keeps at least 3 points
        cuts = [0] + (extra + 3 * np.arange(1, parts)).tolist() + [n]
        out.append([p[b:e].reshape(-1).tolist() for b, e in zip(cuts[:-1], cuts[1:])])
    return out


def points_of(polygons):
    return np.concatenate([np.asarray(p, np.float64) for p in polygons]).reshape(-1, 2)


def as_annotations(polys_list):
    """COCO annotation dicts (non-crowd, a unit bbox that the polygon rules never read) around the generated polygons."""
    return [{"id": i + 1, "image_id": 1, "category_id": 1, "iscrowd": 0, "bbox": [0.0, 0.0, 1.0, 1.0], "segmentation": polys}
            for i, polys in enumerate(polys_list)]


_ORACLE = {}


def generated_with_oracle(count):
    """(generated polygons, their point arrays, min_area_rect of each), computed once per count and shared by the tests."""
    if count not in _ORACLE:
        polys = generate(count)
        pts = [points_of(p) for p in polys]
        _ORACLE[count] = (polys, pts, [min_area_rect(p) for p in pts])
    return _ORACLE[count]


def check_parity(pts_list, oracle, rect, info, cap=0.02, ref_rect=None):
    """The parity rule of the polygon-geometry tests; returns the number of annotations left out of the full-tuple comparison.

    For EVERY annotation: the rectangle encloses all points within 1e-9 * scale, scale = max(1, max |coordinate|); w * h equals the
    oracle's least area within 1e-9 relative (plus what the side tolerance 1e-9 * scale allows, (w + h) * 1e-9 * scale, when
    ``cap`` is None: inputs whose least area is itself rounding noise); min(info, 3) equals min(hull size, 3), and info the hull size
    where the oracle's hull has no three neighbouring vertices with |cross| < 1e-9 * scale^2.
    The five numbers against the oracle's (or ``ref_rect``'s), 1e-9 * scale on cx, cy, w, h and 1e-9 degrees on the angle, unless an
    edge of another direction (more than 1e-6 degrees apart modulo 90) comes within 1e-9 relative of the least area or the angle
    lies within 1e-6 degrees of the fold at +-45.  At most ``cap`` of the annotations may be left out so.
    Both sides do a few dozen float64 operations at 1.1e-16 each (no contraction), so a correct result lies near 1e-13 * scale;
    a wrong edge or a wrong fold shows at 1e-3 or more."""
    rect, info = np.asarray(rect), np.asarray(info)
    assert rect.shape == (len(pts_list), 5) and rect.dtype == np.float64 and info.shape == (len(pts_list),)
    left_out = 0
    for i, (pts, (orect, ohull, edges)) in enumerate(zip(pts_list, oracle)):
        scale = max(1.0, float(np.abs(pts).max()))
        got = rect[i]
        assert np.isfinite(got).all(), (i, got)
        assert encloses(got, pts, 1e-9 * scale), (i, got, orect)
        area = edges[0][0] if edges else orect[2] * orect[3]
        slack = 0.0 if cap is not None else (orect[2] + orect[3]) * 1e-9 * scale
        assert abs(got[2] * got[3] - area) <= 1e-9 * area + slack, (i, got[2] * got[3], area)
        assert min(int(info[i]), 3) == min(ohull, 3), (i, info[i], ohull)
        if not hull_has_near_collinear(pts):
            assert int(info[i]) == ohull, (i, info[i], ohull)
        if is_tie(edges) or abs(abs(orect[4]) - 45.0) <= 1e-6:
            left_out += 1
            continue
        want = orect if ref_rect is None else ref_rect[i]
        assert np.abs(got[:4] - np.asarray(want[:4])).max() <= 1e-9 * scale, (i, got, want)
        assert abs(got[4] - want[4]) <= 1e-9, (i, got, want)
        assert -45.0 < got[4] <= 45.0, (i, got)
    if cap is not None:
        assert left_out <= cap * len(pts_list), (left_out, len(pts_list))
    return left_out
