"""What tests/test_slomo_stream.py (CPU: the fixture and the oracle) and tests/test_slomo_stream_gpu.py (the kernels of
v2e_amd/csrc/slomo_stream.h one by one) share: the shapes, the seeded inputs, and the census of sampling positions of
tests/golden/slomo_stream_edges.npz (written by tests/golden/make_golden_slomo_stream.py, which uses the same census)."""
import numpy as np

TOL = 1e-5   # the suite's bound for float intermediates (tests/test_slomo_gpu.py): |a - b| <= 1e-5 max(1, |b|)


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def rand15(rng, shape, scale=1.0):
    """integer multiples of 2^-15 in [-1, 1), times scale: as the other SloMo tests draw their inputs"""
    return ((rng.integers(0, 1 << 16, size=shape).astype(np.float32) / np.float32(32768.0)) - np.float32(1.0)) * np.float32(scale)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ pooling and bilinear x2: OUTPUT shapes (nc, h, w)
# vector path (w % 4 == 0): one float4 group, several rows, a width of three groups with more than one workgroup's worth of
# channels, a row longer than a workgroup, more planes than one workgroup's 256 groups
POOL_VECTOR = [(3, 1, 4), (2, 3, 8), (5, 17, 12), (1, 1, 260), (2049, 2, 4)]
# scalar path: the 1- and 2-wide levels of a 32-wide input, odd widths, the 6-wide level of a 96-wide input, many workgroups
POOL_SCALAR = [(3, 1, 1), (4, 1, 2), (2, 5, 3), (3, 2, 6), (1, 7, 10), (40960, 1, 1)]
# vector path: sh == 1 (t == 0's second row clamps), one column group (j == 0 is also the last: c1 / c2 clamp), several groups,
# a wide and a tall plane, several workgroups
UP_VECTOR = [(3, 2, 4), (5, 4, 8), (2, 6, 12), (7, 2, 64), (1, 64, 4), (3, 34, 260)]
UP_SCALAR = [(3, 2, 2), (4, 2, 6), (2, 4, 2), (5, 6, 10), (1, 10, 14)]
POOL_SHAPES = POOL_VECTOR + POOL_SCALAR
UP_SHAPES = UP_VECTOR + UP_SCALAR


def pool_input(shape):
    nc, h, w = shape
    rng = np.random.Generator(np.random.PCG64(9000 + nc * 7 + h * 131 + w))
    return rand15(rng, (1, nc, 2 * h, 2 * w), 4.0)


def up_input(shape):
    nc, h, w = shape
    rng = np.random.Generator(np.random.PCG64(9500 + nc * 7 + h * 131 + w))
    return rand15(rng, (1, nc, h // 2, w // 2), 4.0)


F32_MAX = np.float32(3.4028234663852886e38)


def plant_specials(x):
    """+inf, -0.0 and the largest finite float at border pixels of the first plane (and of the last one): a copy of x"""
    x = x.copy()
    p = x[0, 0]
    p[0, 0] = np.inf
    p[0, -1] = np.float32(-0.0)
    p[-1, 0] = F32_MAX
    p[-1, -1] = -F32_MAX
    q = x[0, -1]
    q[-1, q.shape[1] // 2] = np.inf
    q[q.shape[0] // 2, -1] = np.float32(-0.0)
    return x


# ------------------------------------------------------------------ k_amax
# 1 .. 8: the scalar tail alone and beside one or two vectors; 1023 .. 1025: a workgroup's 256 vectors and one element more;
# 262145: many workgroups and a tail; 4197378 = 4 * (4096 * 256 + 512) + 2: past the 4096-workgroup cap (a second grid-stride trip)
AMAX_SIZES = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 262145, 4197378]


def amax_positions(n):
    """where the unique maximum is placed in turn: index 0, the last vector element, every tail element, and past the first
    grid-stride trip (4096 workgroups x 256 lanes x 4 floats) where there is one"""
    n4 = n & ~3
    pos = {0}
    if n4:
        pos.add(n4 - 1)
    pos.update(range(n4, n))
    if n > 4096 * 256 * 4:
        pos.add(4096 * 256 * 4)
        pos.add(n4 - 5)
    return sorted(pos)


# ------------------------------------------------------------------ k_max_speed2 (b, h, w)
# one element; less than a wave; several waves with b > 1; one workgroup per pair exactly; a ragged last workgroup;
# 3 * 352 * 512 = 540 672 vectors = 2112 workgroups' worth, past the 2048-workgroup cap
SPEED_SHAPES = [(1, 1, 1), (1, 3, 5), (3, 7, 9), (2, 16, 16), (5, 17, 31), (3, 352, 512)]


def speed2_ref(flow):
    """max(max(x0*x0 + y0*y0, x1*x1 + y1*y1)) in float32, one rounded operation at a time: uint32 bits (0xffffffff: a NaN)"""
    f = np.asarray(flow, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        s0 = (f[:, 0] * f[:, 0]) + (f[:, 1] * f[:, 1])
        s1 = (f[:, 2] * f[:, 2]) + (f[:, 3] * f[:, 3])
    assert s0.dtype == np.float32
    if np.isnan(s0).any() or np.isnan(s1).any():
        return 0xFFFFFFFF
    return int(np.float32(max(s0.max(), s1.max())).view(np.uint32))


# ------------------------------------------------------------------ warp / blend / fusion fixture
# (h, w, b, n_t): less than a wave; one workgroup exactly; one workgroup and five pixels; several workgroups with b = 3
EDGE_CASES = [(5, 7, 3, 2), (16, 16, 2, 3), (9, 29, 2, 1), (24, 40, 3, 2)]
EDGE_FIXTURE = "slomo_stream_edges.npz"
# every case's ts contains 0.5: the blend coefficients are +-0.25 there, so flows that are multiples of 4 blend to integers and
# multiples of 2 to halves, exactly; 0.25 (coefficients -3/16, 1/16, 9/16) is as exact
EDGE_TS = {1: [0.5], 2: [0.5, 0.25], 3: [0.25, 0.5, 0.75]}
LOGITS = [0.0, 20.0, -20.0, 90.0, -90.0, 110.0, -110.0]   # sigmoid saturates to exactly 0 / 1 in float32 from +-90 on (+-20: 1 - v0 does)
MIN_PER_CLASS = 8


def case_name(case):
    return "h%dw%db%dt%d" % tuple(case)


def load_case(z, case):
    p = case_name(case) + "_"
    d = {k[len(p):]: z[k] for k in z.files if k.startswith(p)}
    fr = d["frames"]
    b = case[2]
    assert fr.shape == (b + 1, case[0], case[1])
    t = (fr.astype(np.float32) / np.float32(255.0))[:, None] - np.float32(0.428)
    d["I0"], d["I1"] = np.ascontiguousarray(t[:b]), np.ascontiguousarray(t[1:b + 1])
    d["ts"] = [float(t) for t in d["ts"]]
    return d


def time_coefficients(ts):
    """fCoeff / wCoeff rows as the host forms them (v2e_amd.planning.time_coefficients)"""
    rows = []
    for t in ts:
        t = float(t)
        temp = -t * (1 - t)
        rows.append([temp, t * t, (1 - t) * (1 - t), temp, 1 - t, t])
    return np.asarray(rows, dtype=np.float64).astype(np.float32)


def classify(ix, iy, h, w):
    """The classes of a bilinear sampling position (ix, iy) in pixel coordinates of an h x w image with zero padding (grid_sample,
    align_corners=False: backWarp's x + flow lands on ix = x + flow - 0.5).  An x class counts only where some row of the
    position has a non-zero weight inside the image (-1 < iy < h), so that a wrong column test changes the sample; likewise y."""
    ix, iy = np.asarray(ix, np.float64), np.asarray(iy, np.float64)
    vis_x, vis_y = (ix > -1) & (ix < w), (iy > -1) & (iy < h)
    whole = lambda v: v == np.floor(v)
    c = {}
    c["interior_integer"] = whole(ix) & whole(iy) & (ix >= 0) & (ix <= w - 2) & (iy >= 0) & (iy <= h - 2)   # tx == ty == 0
    c["x_on_minus_1"] = (ix == -1) & vis_y
    c["x_on_last"] = (ix == w - 1) & vis_y
    c["x_on_size"] = (ix == w) & vis_y
    c["y_on_minus_1"] = (iy == -1) & vis_x
    c["y_on_last"] = (iy == h - 1) & vis_x
    c["y_on_size"] = (iy == h) & vis_x
    c["half_across_left"] = (ix == -0.5) & vis_y
    c["half_across_right"] = (ix == w - 0.5) & vis_y
    c["half_across_top"] = (iy == -0.5) & vis_x
    c["half_across_bottom"] = (iy == h - 0.5) & vis_x
    lo_x, hi_x = (ix > -1) & (ix < 0), (ix > w - 1) & (ix < w)
    lo_y, hi_y = (iy > -1) & (iy < 0), (iy > h - 1) & (iy < h)
    c["corner_top_left"], c["corner_top_right"] = lo_x & lo_y, hi_x & lo_y   # exactly one neighbour inside
    c["corner_bottom_left"], c["corner_bottom_right"] = lo_x & hi_y, hi_x & hi_y
    c["far_below"] = (ix < -1e4) | (iy < -1e4)
    c["far_above"] = (ix > 1e4) | (iy > 1e4)
    return c


CLASSES = tuple(classify(0.0, 0.0, 4, 4))
# far outside is one class of 8, held as 4 on either side
CLASS_MIN = {k: (MIN_PER_CLASS // 2 if k.startswith("far_") else MIN_PER_CLASS) for k in CLASSES}


def _grid(h, w):
    py, px = np.mgrid[0:h, 0:w].astype(np.float64)
    return px, py


def prep_positions(d, case):
    """float64 sampling positions of k_prep from the fixture's own flow: {0: (ix, iy) of g(I0, Ft0), 1: of g(I1, Ft1)}, each
    [n_t][b][h][w]"""
    h, w, b, n_t = case
    c = time_coefficients(d["ts"]).astype(np.float64)
    fl = d["flow"].astype(np.float64)
    px, py = _grid(h, w)
    out = {0: [], 1: []}
    for ti in range(n_t):
        ft0x, ft0y = c[ti, 0] * fl[:, 0] + c[ti, 1] * fl[:, 2], c[ti, 0] * fl[:, 1] + c[ti, 1] * fl[:, 3]
        ft1x, ft1y = c[ti, 2] * fl[:, 0] + c[ti, 3] * fl[:, 2], c[ti, 2] * fl[:, 1] + c[ti, 3] * fl[:, 3]
        out[0].append((px + ft0x - 0.5, py + ft0y - 0.5))
        out[1].append((px + ft1x - 0.5, py + ft1y - 0.5))
    return {k: (np.stack([p[0] for p in v]), np.stack([p[1] for p in v])) for k, v in out.items()}


def fuse_positions(d, case):
    """the same for k_fuse: the refined flows intrp[0:2] + Ft0 (x12 channels 8, 9) and intrp[2:4] + Ft1 (channels 6, 7)"""
    h, w, b, n_t = case
    q, tail = d["intrp"].astype(np.float64), d["x12_tail"].astype(np.float64)   # [n_t][b][5], [n_t][b][6] = channels 6 .. 11
    px, py = _grid(h, w)
    return {0: (px + q[:, :, 0] + tail[:, :, 2] - 0.5, py + q[:, :, 1] + tail[:, :, 3] - 0.5),
            1: (px + q[:, :, 2] + tail[:, :, 0] - 0.5, py + q[:, :, 3] + tail[:, :, 1] - 0.5)}


def census(positions, case):
    """{direction: {class: count}} of prep_positions / fuse_positions"""
    h, w = case[0], case[1]
    return {k: {name: int(m.sum()) for name, m in classify(ix, iy, h, w).items()} for k, (ix, iy) in positions.items()}


def census_short(cen):
    return ["%d:%s=%d" % (k, name, n) for k, c in cen.items() for name, n in c.items() if n < CLASS_MIN[name]]
