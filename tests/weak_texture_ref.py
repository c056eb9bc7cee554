"""A PLAIN STATEMENT of the weak-texture detection (texture_kernels.hip; oracle tsar_oracle_texture.c) and the images that take it off the
axes.  Shared by the CPU test (oracle against the plain statement, test_weak_texture_shapes_cpu.py) and the GPU test (kernels against
both, test_gpu_weak_texture_shapes.py).  No test functions here, no ctypes, no oracle: numpy, and scipy.ndimage.label for the components.

What is stated, from the head of texture_kernels.hip and include/tsar.h:
    8-bit gray -> pyrDown twice (each: size w / 2, h / 2 truncated; the 5x5 [1 4 6 4 1] kernel in integers about the even source
    pixels, borders REFLECT_101, (sum + 128) >> 8) -> Roberts cross, the magnitude cast to uchar (it wraps at 256), the image border
    answering sqrt(2 * 5000) = 100 -> edge where the magnitude exceeds 4 -> [closing] -> border fix (rows pass, then columns pass) ->
    4-connected components of the non-edge pixels, numbered from 1 by the raster position of their first pixel, label 0 = edge pixels ->
    count and bounding box -> weak when count > 5000 and (xs * ys < 2 * count or count > 100000), xs = xmax - xmin, ys = ymax - ymin,
    size = max(xs, ys) -> labels at full resolution, pixel (x, y) reading (x / 4, y / 4), one back where that is past the end.

The closing, for every component of more than 5000 pixels of a first labelling (taken BEFORE the border fix), each on its own:
    boundary  the pixels outside the component with a 4-neighbour inside it;
    votes     every boundary pixel votes once per degree t = 0..179 for rho = rint(x cos t + y sin t): float32 tables, two rounded
              products and one rounded sum, ties to even; a table of 180 x (2 (w4 + h4 + 2) + 1) cells, rho = column - (w4 + h4 + 2);
    peaks     cells with v >= 110, v > left, v >= right (rho - 1, rho + 1), v > up, v >= down (t - 1, t + 1); a missing neighbour is 0,
              t does not wrap;
    walk      along x when |sin| >= |cos|, else along y, one pixel per step over the whole axis, the other coordinate
              rint((rho - k cos) / sin) resp. rint((rho - k sin) / cos) in float32;
    runs      the steps that land on a boundary pixel, grouped: two hits belong to one run when at most 18 steps miss between them (a
              step outside the image misses); a run is drawn when its first and last hit differ by >= 160 in x or in y;
    drawing   the 8-connected Bresenham line from the first hit to the last: err = dx - dy; at every pixel e2 = 2 err, x steps when
              e2 >= -dy (err -= dy), y steps when e2 <= dx (err += dx), both tests on the same e2.
Because a run either meets a 19th miss or the end of the axis, every group is judged exactly once: the walk is stated on the sorted hit
positions, without a step loop.  Runs are reported with the longest gap bridged inside them and the number of misses after them."""
import functools

import numpy as np
from scipy import ndimage

HOUGH_THR, HOUGH_MINLEN, HOUGH_MAXGAP = 110, 160, 18
WEAK_COUNT, WEAK_COUNT_ALWAYS, SIZERAT = 5000, 100000, 2
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def hough_tables():
    a = np.arange(180, dtype=np.float64) * 3.14159265358979323846 / 180.0
    return np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)


# ---- the stages --------------------------------------------------------------------------------------------------------------------
def pyr_down(img):
    h, w = img.shape
    dw, dh = w // 2, h // 2
    p = np.pad(img.astype(np.int64), 2, mode="reflect")                    # numpy's "reflect" is REFLECT_101: the edge pixel is not repeated
    k = (1, 4, 6, 4, 1)
    rows = sum(k[i] * p[:, i:i + 2 * dw:2] for i in range(5))              # [h + 4, dw]
    full = sum(k[j] * rows[j:j + 2 * dh:2] for j in range(5))              # [dh, dw]
    return ((full + 128) >> 8).astype(np.uint8)


def roberts_edges(g):
    s = g.astype(np.int64)
    a = s[:-1, :-1] - s[1:, 1:]
    b = s[1:, :-1] - s[:-1, 1:]
    mag = np.full(g.shape, 100, np.int64)                                   # border: (uchar)sqrt(5000 + 5000)
    inner = np.sqrt((a * a + b * b).astype(np.float64)).astype(np.int64) & 255
    mag[1:-1, 1:-1] = inner[1:, 1:]                                        # pixel (i, j) reads (i + 1, j + 1): rows 1..h-2, columns 1..w-2
    return np.where(mag > 4, 255, 0).astype(np.uint8)


def border_fix(edge):
    e = edge.copy()
    e[e[:, 1] == 0, 0] = 0
    e[e[:, -2] == 0, -1] = 0
    e[0, e[1, :] == 0] = 0                                                  # reads what the rows pass left in rows 1 and h - 2
    e[-1, e[-2, :] == 0] = 0
    return e


def components(edge):
    """[h, w] int32: 0 on edge pixels, else 1 + the number of components whose first pixel comes earlier in raster order"""
    lab, n = ndimage.label(edge == 0, structure=FOUR)
    if n == 0:
        return lab.astype(np.int32), 1
    ids, first = np.unique(lab.ravel(), return_index=True)
    first = first[ids > 0]
    ids = ids[ids > 0]
    new = np.zeros(n + 1, np.int32)
    new[ids[np.argsort(first, kind="stable")]] = np.arange(1, n + 1)
    return new[lab], n + 1


def bresenham(x0, y0, x1, y1):
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx - dy
    out = []
    while True:
        out.append((x0, y0))
        if x0 == x1 and y0 == y1:
            return out
        e2 = 2 * err
        if e2 >= -dy:
            err -= dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def hough_close(edge):
    """-> (edge with the kept runs drawn, number drawn, runs): runs is a list of dicts t, rho, xmajor, start (x, y), end (x, y), hits,
    max_gap (the longest gap bridged inside the run), end_gap (the misses after its last hit: up to the next hit, or to the end of the
    axis), at_axis_end, drawn, component (size of the first-labelling component)"""
    h, w = edge.shape
    cs, sn = hough_tables()
    lab0, n0 = components(edge)
    cnt0 = np.bincount(lab0.ravel(), minlength=n0)
    rmax = w + h + 2
    nrho = 2 * rmax + 1
    out = edge.copy()
    runs = []
    for L in range(1, n0):
        if cnt0[L] <= WEAK_COUNT:
            continue
        comp = lab0 == L
        near = np.zeros_like(comp)
        near[:, 1:] |= comp[:, :-1]
        near[:, :-1] |= comp[:, 1:]
        near[1:, :] |= comp[:-1, :]
        near[:-1, :] |= comp[1:, :]
        bmask = near & ~comp
        ys, xs = np.nonzero(bmask)
        xf, yf = xs.astype(np.float32), ys.astype(np.float32)
        acc = np.zeros((180, nrho), np.int64)
        for t in range(180):
            rho = np.rint(xf * cs[t] + yf * sn[t]).astype(np.int64)        # float32 throughout: products and sum each round once
            acc[t] = np.bincount(rho + rmax, minlength=nrho)
        z = np.pad(acc, 1)
        v = z[1:-1, 1:-1]
        peak = (v >= HOUGH_THR) & (v > z[1:-1, :-2]) & (v >= z[1:-1, 2:]) & (v > z[:-2, 1:-1]) & (v >= z[2:, 1:-1])
        for t, r in zip(*np.nonzero(peak)):
            c, s, rho = cs[t], sn[t], np.float32(r - rmax)
            xmajor = bool(abs(s) >= abs(c))
            n = w if xmajor else h
            k = np.arange(n)
            kf = k.astype(np.float32)
            other = np.rint((rho - kf * c) / s if xmajor else (rho - kf * s) / c).astype(np.int64)
            x, y = (k, other) if xmajor else (other, k)
            inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            hit = np.zeros(n, bool)
            hit[inside] = bmask[y[inside], x[inside]]
            at = np.nonzero(hit)[0]
            if len(at) == 0:
                continue
            gaps = np.diff(at) - 1                                          # misses between consecutive hits
            cuts = np.nonzero(gaps > HOUGH_MAXGAP)[0]
            lo = np.concatenate(([0], cuts + 1))
            hi = np.concatenate((cuts, [len(at) - 1]))
            for a, b in zip(lo, hi):
                k0, k1 = at[a], at[b]
                p0, p1 = (int(x[k0]), int(y[k0])), (int(x[k1]), int(y[k1]))
                last = b == len(at) - 1
                keep = abs(p1[0] - p0[0]) >= HOUGH_MINLEN or abs(p1[1] - p0[1]) >= HOUGH_MINLEN
                runs.append(dict(t=int(t), rho=int(r - rmax), xmajor=xmajor, start=p0, end=p1, hits=int(b - a + 1),
                                 max_gap=int(gaps[a:b].max()) if b > a else 0, end_gap=int(n - 1 - k1) if last else int(gaps[b]),
                                 at_axis_end=bool(last), drawn=bool(keep), component=int(cnt0[L])))
                if keep:
                    for px, py in bresenham(*p0, *p1):
                        if 0 <= px < w and 0 <= py < h:
                            out[py, px] = 255
    return out, sum(r["drawn"] for r in runs), runs


def region_stats(lab, n):
    h, w = lab.shape
    yy, xx = np.mgrid[0:h, 0:w]
    l = lab.ravel()
    count = np.bincount(l, minlength=n).astype(np.int64)
    xmin, ymin = np.full(n, w - 1), np.full(n, h - 1)
    xmax, ymax = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.minimum.at(xmin, l, xx.ravel()); np.maximum.at(xmax, l, xx.ravel())
    np.minimum.at(ymin, l, yy.ravel()); np.maximum.at(ymax, l, yy.ravel())
    xs, ys = xmax - xmin, ymax - ymin
    weak = (count > WEAK_COUNT) & ((xs * ys < SIZERAT * count) | (count > WEAK_COUNT_ALWAYS))
    weak[0] = False
    text = np.where(weak, -1.0, 1.0).astype(np.float32)
    size = np.where(weak, np.maximum(xs, ys), 0).astype(np.float32)
    return count.astype(np.int32), text, size, xs, ys


def upsample(lab4, w, h):
    h4, w4 = lab4.shape
    sx, sy = np.arange(w) // 4, np.arange(h) // 4
    sx = np.where(sx >= w4, sx - 1, sx)
    sy = np.where(sy >= h4, sy - 1, sy)
    return lab4[sy[:, None], sx[None, :]]


def weak_texture(gray_u8, close_lines=True):
    """-> dict(labels4, labels, text, size, count, edge, segments, runs, count0, xs, ys); count0 = sizes of the first labelling's
    components above 5000, ascending"""
    g = np.ascontiguousarray(gray_u8, np.uint8)
    h, w = g.shape
    edge = roberts_edges(pyr_down(pyr_down(g)))
    lab0, n0 = components(edge)
    c0 = np.bincount(lab0.ravel(), minlength=n0)[1:]
    segments, runs = 0, []
    if close_lines:
        edge, segments, runs = hough_close(edge)
    edge = border_fix(edge)
    lab4, n = components(edge)
    count, text, size, xs, ys = region_stats(lab4, n)
    return dict(labels4=lab4, labels=upsample(lab4, w, h), text=text, size=size, count=count, edge=edge, segments=segments, runs=runs,
                count0=np.sort(c0[c0 > WEAK_COUNT]), xs=xs, ys=ys)


# ---- the images --------------------------------------------------------------------------------------------------------------------
FLAT = 120


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w)).astype(np.uint8)


def band_image(w, h, deg, gap=40, band=40, margin=40, seed=0):
    """noise; flat inside the margin, except in a noise band of width `band` about the line through the centre with direction `deg`,
    which a flat gap of length `gap` pierces at the centre"""
    img = _noise(w, h, seed)
    a = np.deg2rad(float(deg))
    yy, xx = np.mgrid[0:h, 0:w]
    dx, dy = xx - w / 2.0, yy - h / 2.0
    inside = (xx >= margin) & (xx < w - margin) & (yy >= margin) & (yy < h - margin)
    across = np.abs(-dx * np.sin(a) + dy * np.cos(a))
    along = np.abs(dx * np.cos(a) + dy * np.sin(a))
    img[inside & ((across > band / 2.0) | (along < gap / 2.0))] = FLAT
    return img


def two_bands(w=1303, h=1001):
    """two banded areas side by side, a noise wall between them: two large components in the first labelling"""
    img = _noise(w, h, 3)
    img[:, :640] = band_image(640, h, 60, seed=4)
    img[:, w - 640:] = band_image(640, h, 120, seed=5)
    return img


def serpentine(w, h, cor=24, wall=24, margin=40, seed=6):
    """horizontal flat corridors of height `cor`, `wall` apart, joined alternately at the right and at the left end: one long chain"""
    img = _noise(w, h, seed)
    n = (h - 2 * margin + wall) // (cor + wall)
    for i in range(n):
        y0 = margin + i * (cor + wall)
        img[y0:y0 + cor, margin:w - margin] = FLAT
        if i + 1 < n:
            x0 = w - margin - cor if i % 2 == 0 else margin
            img[y0 + cor:y0 + cor + wall, x0:x0 + cor] = FLAT
    return img


def comb(w=902, h=701, teeth=14, cor=24, margin=40, seed=7):
    """vertical flat teeth of width `cor`, evenly spread, joined by a spine of height `cor` along the BOTTOM: in raster order every
    tooth is met on its own for all of its length and meets the others last"""
    img = _noise(w, h, seed)
    img[h - margin - cor:h - margin, margin:w - margin] = FLAT
    for i in range(teeth):
        x0 = margin + (w - 2 * margin - cor) * i // (teeth - 1)
        img[margin:h - margin, x0:x0 + cor] = FLAT
    return img


def spiral(w=902, h=701, turns=14, cor=24, wall=24, margin=40, seed=8):
    """one rectangular spiral corridor of width `cor`, `wall` between its windings, `turns` straight legs from the outside inwards"""
    img = _noise(w, h, seed)
    x0, y0, x1, y1 = margin, margin, w - margin, h - margin             # the free box, shrunk as the legs are laid
    step = cor + wall
    for i in range(turns):
        side = i % 4
        if side == 0:                                                    # along the top, left to right
            img[y0:y0 + cor, (x0 - step if i else x0):x1] = FLAT     # from the leg that came up the left side
            y0 += step
        elif side == 1:                                                  # down the right side
            img[y0 - step:y1, x1 - cor:x1] = FLAT
            x1 -= step
        elif side == 2:                                                  # along the bottom, right to left
            img[y1 - cor:y1, x0:x1 + step] = FLAT
            y1 -= step
        else:                                                            # up the left side
            img[y0:y1 + step, x0:x0 + cor] = FLAT
            x0 += step
        assert x1 - x0 >= cor and y1 - y0 >= cor, "too many turns for this size"
    return img


def stripe_case(w, h, hole, length=None, top=None, band=40, margin=40, seed=9):
    """flat inside the margin but for a vertical noise stripe of width `band` and `length` pixels (default: the whole flat height; about
    the centre, or from row `top` down), with a flat hole of `hole` pixels about the image's middle row"""
    img = _noise(w, h, seed)
    img[margin:h - margin, margin:w - margin] = FLAT
    stripe = _noise(w, h, seed + 1)
    length = h - 2 * margin if length is None else length
    ya = h // 2 - length // 2 if top is None else top
    xa = w // 2 - band // 2
    img[ya:ya + length, xa:xa + band] = stripe[ya:ya + length, xa:xa + band]
    yh = h // 2 - hole // 2
    img[yh:yh + hole, xa:xa + band] = FLAT
    return img


def count_case(w, h, rw, rh, pw=0, ph=0, block=None, seed=10):
    """one flat rectangle of 4 rw x 4 rh pixels at (40, 40) with a flat protrusion of 4 pw x 4 ph pixels on its right side, top-aligned;
    block = (bx, by): one 4 x 4 noise block at that quarter-resolution offset inside the protrusion"""
    img = _noise(w, h, seed)
    img[40:40 + 4 * rh, 40:40 + 4 * rw] = FLAT
    img[40:40 + 4 * ph, 40 + 4 * rw:40 + 4 * (rw + pw)] = FLAT
    if block is not None:
        bx, by = 40 + 4 * (rw + block[0]), 40 + 4 * block[1]
        img[by:by + 4, bx:bx + 4] = _noise(w, h, seed + 1)[by:by + 4, bx:bx + 4]
    return img


def ell_case(w, h, aw, ah, bw, bh, pw=0, ph=0, seed=11):
    """a flat L at (40, 40): a vertical arm of 4 aw x 4 ah pixels and, along its foot, a horizontal arm of 4 bw x 4 bh pixels to its right;
    a flat protrusion of 4 pw x 4 ph pixels on the vertical arm's right side, top-aligned, adds pixels inside the bounding box"""
    img = _noise(w, h, seed)
    img[40:40 + 4 * ph, 40 + 4 * aw:40 + 4 * (aw + pw)] = FLAT
    img[40:40 + 4 * ah, 40:40 + 4 * aw] = FLAT
    img[40 + 4 * (ah - bh):40 + 4 * ah, 40 + 4 * aw:40 + 4 * (aw + bw)] = FLAT
    return img


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
BAND_DEGREES = (0, 30, 45, 60, 83, 90, 97, 120, 135, 150, 173)
GAP_PAIR = ("stripe_hole72", "stripe_hole76")          # the x = 69 side of the stripe: a gap of 18 bridged | the run ended by a gap of 19
LEN_PAIR = ("stripe_len644", "stripe_len640")          # a side run of 160 kept | the longest side run 159, dropped
COUNT_PAIR = ("count5000", "count5001")                # one 4 x 4 noise block apart
BOX_PAIR = ("box_equal", "box_below")                  # xs ys = 134 * 133 = 17822 = 2 * 8911 | 17822 < 2 * 8912; the protrusion one quarter-pixel taller

CASES = {"band%d" % d: (lambda d=d: band_image(902, 1001, d)) for d in BAND_DEGREES}
CASES.update({
    "band7": lambda: band_image(902, 1001, 7),
    "short900x700_45": lambda: band_image(900, 700, 45),
    "short901x703_135": lambda: band_image(901, 703, 135),
    "two_bands": two_bands,
    "serpentine902": lambda: serpentine(902, 1001),
    "serpentine1203": lambda: serpentine(1203, 1001),
    "comb": lambda: comb(902, 801),
    "spiral": spiral,
    "stripe_hole72": lambda: stripe_case(600, 900, 72),
    "stripe_hole76": lambda: stripe_case(600, 900, 76),
    "stripe_len644": lambda: stripe_case(600, 900, 24, 644, top=123),
    "stripe_len640": lambda: stripe_case(600, 900, 24, 640, top=123),
    "count5000": lambda: count_case(384, 460, 66, 78, 3, 18, block=(0, 14)),
    "count5001": lambda: count_case(384, 460, 66, 78, 3, 18),
    "box_equal": lambda: ell_case(640, 640, 43, 132, 89, 40, 2, 39),
    "box_below": lambda: ell_case(640, 640, 43, 132, 89, 40, 2, 40),
    "sawtooth": lambda: sawtooth(600, 1200, 64, 44, 860),
})


@functools.lru_cache(maxsize=None)
def image(name):
    img = CASES[name]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def plain(name, close_lines):
    """the plain statement's result for a case, computed once per process and left unchanged"""
    return weak_texture(image(name), close_lines=close_lines)


def stripe_side_runs(res, w=600, band=40):
    """the walk's runs along the two long sides of stripe_case's stripe: vertical lines whose ends lie within 2 pixels of it"""
    xa = (w // 2 - band // 2) / 4.0
    near = lambda x: xa - 2 <= x <= xa + band / 4.0 + 2
    return [r for r in res["runs"] if not r["xmajor"] and near(r["start"][0]) and near(r["end"][0])]


def sawtooth(w, h, period=64, inn=32, rows=None, margin=40, seed=12):
    """flat inside the margin, the right side stepped 4 pixels in for the last `inn` rows of every `period` (the first `rows` rows of the
    flat area are shaped, default all): the right boundary's votes at 0 degrees fall into two neighbouring rho cells"""
    img = _noise(w, h, seed)
    img[margin:h - margin, margin:w - margin] = FLAT
    back = _noise(w, h, seed + 1)
    for y in range(margin, h - margin if rows is None else margin + rows):
        if (y - margin) % period >= period - inn:
            img[y, w - margin - 4:w - margin] = back[y, w - margin - 4:w - margin]
    return img
