"""The image pyramid of the coarse-to-fine mode (tsar_pyramid_views, include/tsar.h) restated in numpy, with known answers, and the
coarse level's camera (K / 2) checked against the CPU oracle.  No GPU: the GPU tests (test_gpu_multiscale.py) hold the device's
pyramid to `pyr_down` below bit for bit.

The filter is OpenCV's pyrDown: [1 4 6 4 1]^T [1 4 6 4 1] / 256 centred on source pixel (2x, 2y), BORDER_REFLECT_101, output
((w + 1) / 2, (h + 1) / 2).  8-bit views: integer sums, (s + 128) >> 8.  Float views: per source row (((t0 + 4 t1) + 6 t2) + 4 t3) + t4,
then the same over the five row sums, times 1/256, in float32."""
import numpy as np
import pytest

KW = np.array([1, 4, 6, 4, 1], np.int64)


def reflect101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(img, u8):
    """one pyramid level of a [h, w] view; u8: the view is an 8-bit decode (returns uint8), else float32 arithmetic (returns float32)"""
    img = np.asarray(img)
    h, w = img.shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    xs = [reflect101(2 * np.arange(cw) - 2 + i, w) for i in range(5)]
    ys = [reflect101(2 * np.arange(ch) - 2 + j, h) for j in range(5)]
    if u8:
        a = img.astype(np.int64)
        s = sum(KW[j] * sum(KW[i] * a[ys[j]][:, xs[i]] for i in range(5)) for j in range(5))
        return ((s + 128) >> 8).astype(np.uint8)
    a = img.astype(np.float32)
    f4, f6 = np.float32(4), np.float32(6)

    def comb(t):
        r = t[0] + f4 * t[1]
        r = r + f6 * t[2]
        r = r + f4 * t[3]
        return r + t[4]
    rows = [comb([a[ys[j]][:, xs[i]] for i in range(5)]) for j in range(5)]
    return (comb(rows) * np.float32(1.0 / 256.0)).astype(np.float32)


def coarse_K(K):
    """the coarse level's intrinsics: fx, fy, cx, cy halved (include/tsar.h tsar_pyramid_views)"""
    Kc = np.array(K, np.float32, copy=True)
    Kc[..., 0, 0] *= 0.5
    Kc[..., 0, 2] *= 0.5
    Kc[..., 1, 1] *= 0.5
    Kc[..., 1, 2] *= 0.5
    return Kc


def _padded_sum(img):
    """independent form: pad by two with numpy's 'reflect' (= REFLECT_101), then the 25-tap sum at every (2x, 2y)"""
    h, w = img.shape
    P = np.pad(img.astype(np.int64), 2, mode="reflect")
    cw, ch = (w + 1) // 2, (h + 1) // 2
    s = np.zeros((ch, cw), np.int64)
    for j in range(5):
        for i in range(5):
            s += KW[j] * KW[i] * P[j:j + 2 * ch:2, i:i + 2 * cw:2]
    return s


@pytest.mark.parametrize("u8", [True, False])
def test_constant_image_stays_constant(u8):
    for v in (0, 1, 77, 255):
        img = np.full((13, 10), v, np.uint8 if u8 else np.float32)
        out = pyr_down(img, u8)
        assert out.shape == (7, 5) and (out == v).all()
    img = np.full((9, 12), 3.3125, np.float32)         # a float that stays exact through the sums
    assert (pyr_down(img, False) == np.float32(3.3125)).all()


def test_impulse_response_is_the_binomial_outer_product():
    """coarse pixel (x0, y0) as a function of where a unit impulse sits in the source: [1 4 6 4 1] / 16 outer itself, centred on
    (2 x0, 2 y0)"""
    want = np.outer(KW, KW).astype(np.float64) / 256.0
    x0, y0 = 5, 4
    got = np.zeros((5, 5))
    for j in range(5):
        for i in range(5):
            img = np.zeros((20, 24), np.float32)
            img[2 * y0 - 2 + j, 2 * x0 - 2 + i] = 1.0
            out = pyr_down(img, False)
            got[j, i] = out[y0, x0]
            assert np.count_nonzero(out) <= 9                    # an impulse reaches at most 3 x 3 coarse pixels
    assert np.array_equal(got, want)
    assert np.isclose(want.sum(), 1.0) and np.array_equal(want, np.outer(KW / 16.0, KW / 16.0))


@pytest.mark.parametrize("shape", [(64, 96), (65, 97), (9, 9), (8, 8), (33, 48), (17, 10)])
def test_reflect101_borders_and_odd_even_sizes(shape):
    """every border of odd and even sizes: the integer sums equal the padded form's; output size ((w + 1) / 2, (h + 1) / 2)"""
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape).astype(np.uint8)
    s = _padded_sum(img)
    h, w = shape
    assert s.shape == ((h + 1) // 2, (w + 1) // 2)
    assert np.array_equal(pyr_down(img, True), ((s + 128) >> 8).astype(np.uint8))
    # the float path of an integral image: the sums are exact (< 2^24), so only the final scaling rounds
    assert np.array_equal(pyr_down(img.astype(np.float32), False), (s.astype(np.float64) / 256.0).astype(np.float32))
    # the border rule itself: reflection excludes the edge pixel (gfedcb|abcdefgh|gfedcba)
    assert list(reflect101(np.array([-2, -1, 0, w - 1, w, w + 1]), w)) == [2, 1, 0, w - 1, w - 2, w - 3]
    # a ramp along x: the reflected left border pulls the first coarse pixel up, not towards zero
    ramp = np.tile(np.arange(w, dtype=np.float32), (h, 1))
    assert pyr_down(ramp, False)[0, 0] == np.float32((6 * 0 + 2 * 4 * 1 + 2 * 1 * 2) / 16.0)


def test_u8_rounding_at_exact_halves():
    """(s + 128) >> 8 rounds a sum of exactly k + 0.5 (x 256) up, and anything below it down"""
    img = np.zeros((16, 16), np.uint8)
    img[8, 8] = 32                         # centre tap: s = 36 * 32 = 1152 = 4.5 * 256
    assert pyr_down(img, True)[4, 4] == 5
    img[8, 8] = 7                          # s = 252 -> 0.984 -> 1
    assert pyr_down(img, True)[4, 4] == 1
    img[:] = 0
    img[8, 9] = 32                         # tap weight 24 at (4, 4) and (5, 4): s = 768 = 3.0 * 256
    assert pyr_down(img, True)[4, 4] == 3
    img[:] = 0
    img[9, 9] = 8                          # weight 16: s = 128 = exactly 0.5 -> 1 (half up), in the 4 coarse pixels it reaches
    out = pyr_down(img, True)
    assert out[4, 4] == 1 and out[5, 5] == 1 and out[4, 5] == 1 and out[5, 4] == 1
    img[9, 9] = 7                          # s = 112 < 128 -> 0
    assert pyr_down(img, True).max() == 0


def test_coarse_camera_against_the_oracle():
    """the coarse level of a synthetic scene (pyrDown of its 8-bit views, K / 2): in the reference's arithmetic the oracle scores the
    ground-truth planes far below random ones — and below the same planes under the fine level's K, which would be the wrong camera"""
    import oracle_lib as ol
    from tsar_mvs_amd import synth
    sc = synth.make_scene(192, 128, 3, seed=31)
    imgs = [pyr_down(im.numpy().astype(np.uint8), True).astype(np.float32) for im in sc.images]
    ch, cw = imgs[0].shape
    Kc = coarse_K(sc.K)
    gt = synth.gt_planes(sc).numpy()[0::2, 0::2][:ch, :cw]        # coarse pixel (x, y) sits on fine pixel (2x, 2y); planes are metric
    gt = np.ascontiguousarray(gt)
    orc = ol.Oracle(imgs, Kc, sc.R, sc.t, sc.depth_min, sc.depth_max, box=11, n_best=1, seed=3)
    c_gt, _, _ = orc.pm_cost_planes(gt)
    orc.pm_init()
    c_rand = orc.c.copy()
    wrong = ol.Oracle(imgs, sc.K, sc.R, sc.t, sc.depth_min, sc.depth_max, box=11, n_best=1, seed=3)
    c_wrong, _, _ = wrong.pm_cost_planes(gt)
    ok = (c_gt < 2.0) & (c_rand < 2.0) & (c_wrong < 2.0)
    assert ok.mean() > 0.5
    m_gt, m_rand, m_wrong = (float(np.median(c[ok])) for c in (c_gt, c_rand, c_wrong))
    assert m_gt < 0.5 * m_rand, (m_gt, m_rand)
    assert m_gt < m_wrong, (m_gt, m_wrong)
