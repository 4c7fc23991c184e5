"""The numeric contract over its whole domain: hk_device_math.hpp against oracle/hk_oracle_math.h bit for bit (GPU), and the
oracle against IEEE arithmetic (numpy) where the contract IS IEEE arithmetic (CPU).  tests/test_math_contract.py samples the
ranges a frame produces; this module sweeps every exponent, the specials and the edges built for each routine.

Routine of hk_device_math.hpp -> hk_debug_math op -> GPU test here
  sin_, cos_, exp_, exp2_, log2_, pow_, fmin_, fmax_, a / b, sqrtf (0..7, 9, 10)   test_device_ops_0_to_10_over_the_domain
  f32_to_f16 / f16_to_f32 (8)                             test_device_f16_boundaries_three_way
  f32_to_f16's asm barrier, f16(a * b) (30)               test_device_f16_of_a_product_rounds_twice
  sincos_ (21, 22)                                        test_device_sincos_is_sin_and_cos
  exp_nonpositive_ (23)                                   test_device_exp_nonpositive_is_exp
  quotient_by_reciprocal (24)                             test_device_quotient_by_reciprocal
  exp_nonpositive_(quotient_by_reciprocal(..)) (25)       test_device_denoise_weight_is_exp_of_the_ieee_quotient
  pow2_, pow5_, pow16_, pow_quarter_ (26..29)             test_device_constant_powers
  unorm16, snorm8 (31, 32)                                test_device_norm_encoders_at_their_ties
  unpack2x16unorm / unsnorm8 / unorm8, div_norm (14, 15, 20)   test_math_contract.py::test_device_norm_decodes_exhaustive
  f32_to_u32, f32_to_i32 (33, 34)                         test_device_saturating_conversions
  saturate, clamp_ (11, 12, 13), shading / env_brdf (16..19)   test_device_clamps_and_shading
  dot(f3), dot(f4), cross, normalize, mul(mat3), 4x4 mul, length, mix, fract (35..52)   test_device_vector_ops_in_contract_order
  (pack2x16float / unpack2x16float / pack_f16x4 / pack2x16unorm / pack4x8snorm only shift and OR the codes above.)

Limits of what this proves
  * k_debug_math compiles each routine in a context of its own.  Inside a real kernel a fusion across a call boundary can still
    differ; the frame-parity tests (tests/test_parity_gpu.py and its siblings) remain the check for that.
  * The device-side expectations (saturating v_cvt_i32_f32 / v_cvt_u32_f32, IEEE division and square root with denormals kept
    under the build's flags) were read from the code when these tests were written; the GPU tests are what measures them.
"""
import numpy as np
import pytest

from test_math_contract import OPS, edge_inputs
from test_math_contract import oracle_math as orc  # orc_debug_math by op code, in the layout Engine.debug_math takes

f32, f64, u32 = np.float32, np.float64, np.uint32
NEW = {"sincos_sin": 21, "sincos_cos": 22, "exp_nonpositive": 23, "quotient": 24, "denoise_weight": 25, "pow2": 26, "pow5": 27, "pow16": 28,
       "pow_quarter": 29, "f16_product": 30, "unorm16": 31, "snorm8": 32, "to_u32": 33, "to_i32": 34, "dot3": 35, "dot4": 36, "cross": (37, 38, 39),
       "normalize": (40, 41, 42), "mul3": (43, 44, 45), "mul4": (46, 47, 48, 49), "length": 50, "mix": 51, "fract": 52}
TINY = f32(2.0 ** -126)


# ----------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def eng():
    import bevy_hikari_amd as hk

    return hk.Engine(device=0)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(u32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=u32).view(f32)


def assert_same(got, want, what, args=(), nan_equal=True):
    """Bit for bit; two NaNs are equal (the rule of test_math_contract.py) unless the 32 bits are an integer result."""
    same = bits(got) == bits(want)
    if nan_equal:
        same |= np.isnan(got) & np.isnan(want)
    if not same.all():
        i = np.nonzero(~same)[0][:6]
        shown = [np.asarray(a)[i] for a in args]
        raise AssertionError(f"{what}: {(~same).sum()} of {same.size} differ, e.g. inputs={shown} "
                             f"bits={[bits(np.asarray(a, dtype=f32)[i]) for a in args if np.asarray(a).ndim == 1]} got={got[i]} ({bits(got[i])}) want={want[i]} ({bits(want[i])})")


def around(v, k=2):
    """v and its k f32 neighbours either side."""
    v = np.atleast_1d(np.asarray(v, dtype=f32))
    out, up, dn = [v], v, v
    with np.errstate(over="ignore"):  # (the neighbour above the largest finite value is inf)
        for _ in range(k):
            up = np.nextafter(up, f32(np.inf))
            dn = np.nextafter(dn, f32(-np.inf))
            out += [up, dn]
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------------ the shared generator
MANTISSAS = np.array([0, 1, 2, 0x400000, 0x7FFFFE, 0x7FFFFF], dtype=u32)


def unary_domain(per_exponent=4000, seed=101):
    """Both signs x all 256 exponents x (MANTISSAS + per_exponent seeded random mantissas): every shape of subnormal, +-0, +-inf,
    quiet and signalling NaNs (exponent 255: mantissa bit 22 set / clear) included.  2 x 256 x 4006 = 2.05 million values."""
    rng = np.random.default_rng(seed)
    m = np.concatenate([np.broadcast_to(MANTISSAS, (256, MANTISSAS.size)), rng.integers(0, 1 << 23, (256, per_exponent), dtype=u32)], axis=1)
    pos = (np.arange(256, dtype=u32)[:, None] << 23 | m).ravel()
    x = from_bits(np.concatenate([pos, pos | u32(0x80000000)]))
    assert np.isnan(x).any() and np.isinf(x).any() and ((np.abs(x) < TINY) & (x != 0)).sum() > 2 * per_exponent
    return x


def binary_domain(seed=102):
    """The cross product of a smaller such set (2 signs x 256 exponents x mantissas 0, 1, 0x7fffff and one random) with itself:
    2048^2 = 4.2 million pairs."""
    rng = np.random.default_rng(seed)
    m = np.stack([np.zeros(256, u32), np.ones(256, u32), np.full(256, 0x7FFFFF, u32), rng.integers(0, 1 << 23, 256, dtype=u32)], axis=1)
    pos = (np.arange(256, dtype=u32)[:, None] << 23 | m).ravel()
    v = from_bits(np.concatenate([pos, pos | u32(0x80000000)]))
    a, b = np.meshgrid(v, v, indexing="ij")
    return a.ravel().copy(), b.ravel().copy()


def division_edges(seed=103, n=100_000):
    """Pairs on the edges of a / b: subnormal operands, subnormal quotients (exact ties of the subnormal grid included), quotients
    that overflow (and sit either side of the largest finite value), and every combination of the specials and signed zeros."""
    rng = np.random.default_rng(seed)
    A, B = [], []
    sub = from_bits(rng.integers(1, 1 << 23, n, dtype=u32))
    A += [sub, np.exp(rng.uniform(-30, 30, n)).astype(f32), sub]
    B += [np.exp(rng.uniform(-30, 30, n)).astype(f32), sub, from_bits(rng.integers(1, 1 << 23, n, dtype=u32))]
    # exact ties: a = M 2^-149 (normal, 24-bit M) over 2^j leaves M 2^-j on the 2^-149 grid; the bits shifted out are 100..0
    for j in range(1, 25):
        M = rng.integers(1 << 23, 1 << 24, 2000, dtype=np.int64)
        M = (M >> j << j) | (1 << (j - 1))
        A.append((M.astype(f64) * 2.0 ** -149).astype(f32))
        B.append(np.full(M.size, 2.0 ** j, dtype=f32))
    # the same through a denominator whose reciprocal is not exact: a = 3 (2K+1) 2^-149 over 6 = (2K+1) 2^-150, a tie of the grid
    K = np.concatenate([np.arange(0, 4096), rng.integers(0, (1 << 22) // 3, 20000)]).astype(f64)
    for odd, k in ((3, 1), (5, 1), (7, 1), (3, 2), (5, 3), (3, 20), (7, 40)):  # d = odd 2^k, quotient (2K+1) 2^-150
        A.append((odd * (2 * K + 1) * 2.0 ** (k - 1 - 150)).astype(f32))
        B.append(np.full(K.size, odd * 2.0 ** k, dtype=f32))
    A += [np.exp(rng.uniform(-87.3, -40, n)).astype(f32) * rng.choice([-1, 1], n).astype(f32), np.exp(rng.uniform(40, 88.7, n)).astype(f32)]
    B += [np.exp(rng.uniform(0, 60, n)).astype(f32), np.exp(rng.uniform(-100, -1, n)).astype(f32) * rng.choice([-1, 1], n).astype(f32)]
    big = around(np.float32(3.4028234663852886e38), 64)
    big = big[np.isfinite(big)]
    one = around(np.float32(1.0), 64)
    g = np.meshgrid(big, one, indexing="ij")
    A.append(g[0].ravel()); B.append(g[1].ravel())
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45, 1e-38, -1e-38, 3e38, -3e38], dtype=f32)
    g = np.meshgrid(sp, sp, indexing="ij")
    A.append(g[0].ravel()); B.append(g[1].ravel())
    a, b = np.concatenate(A).astype(f32), np.concatenate(B).astype(f32)
    with np.errstate(all="ignore"):
        q = a / b
    assert ((np.abs(q) < TINY) & (q != 0)).sum() > 100_000 and np.isinf(q[np.isfinite(a) & (b != 0)]).sum() > 10_000
    return a, b


def reciprocal_adversaries(seed=104, n=200_000):
    """Numerators built to land the quotient on a rounding boundary of f32: for a boundary m (the midpoint of two neighbouring f32
    values, exact in f64) and a denominator d, x = RN32(m d) and its neighbours.  Normal boundaries over the whole exponent range,
    and boundaries t 2^-150 (t odd) of the subnormal grid - which d = odd 2^k reaches EXACTLY (x = odd t 2^(k-150))."""
    rng = np.random.default_rng(seed)
    X, D = [], []
    K = rng.integers(1 << 23, 1 << 24, n).astype(f64)
    e = rng.integers(-126, 100, n).astype(f64)
    m = (2 * K + 1) * 2.0 ** (e - 24)
    d = (rng.integers(1 << 23, 1 << 24, n).astype(f64) * 2.0 ** rng.integers(-50, 3, n)).astype(f32)
    Ks = rng.integers(0, 1 << 23, n).astype(f64)
    ms = (2 * Ks + 1) * 2.0 ** -150
    ds = (rng.integers(1 << 23, 1 << 24, n).astype(f64) * 2.0 ** rng.integers(-23, 60, n)).astype(f32)
    for mm, dd in ((m, d), (ms, ds)):
        x0 = (mm * dd.astype(f64)).astype(f32)  # the f64 product of a 25-bit and a 24-bit number is exact: one rounding
        for x in (x0, np.nextafter(x0, f32(np.inf)), np.nextafter(x0, f32(-np.inf))):
            X += [x, -x]
            D += [dd, dd]
    # every odd t < 2048 over every odd multiplier < 1024: d = odd 2^k, x = t odd 2^(k-150) (subnormal for k = 1), quotient t 2^-150.
    # Whether the reciprocal's error survives the f64 product's own rounding depends on both mantissas: about 6 % of these differ.
    odd, t = (g.ravel() for g in np.meshgrid(np.arange(3, 1024, 2, dtype=f64), np.arange(1, 2048, 2, dtype=f64), indexing="ij"))
    for k in (1, 30, 100):
        x0, dd = (t * odd * 2.0 ** (k - 150)).astype(f32), (odd * 2.0 ** k).astype(f32)
        assert (x0.astype(f64) / dd.astype(f64) == t * 2.0 ** -150).all()  # exactly on a tie of the subnormal grid
        X += [x0, -x0]
        D += [dd, dd]
    return np.concatenate(X).astype(f32), np.concatenate(D).astype(f32)


def denoise_domain(seed=105, n=2_000_000):
    """kernels_denoise.hip: a = the difference of two f16-representable luminances, b > 0 from 1e-6 up to 7e4."""
    rng = np.random.default_rng(seed)
    lum = rng.integers(0, 0x7C00, (2, n), dtype=np.uint16).view(np.float16).astype(f32)
    a = lum[0] - lum[1]
    b = np.exp(rng.uniform(np.log(1e-6), np.log(7e4), n)).astype(f32)
    b[:4] = [1e-6, 7e4, 1.0, 65504.0]
    return a, b


def quotient_pairs():
    parts = [binary_domain(), division_edges(), reciprocal_adversaries(), denoise_domain(n=500_000)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def reciprocal_emulation(x, d):
    """quotient_by_reciprocal in numpy: RN32(f64(x) * RN64(1 / f64(d)))."""
    with np.errstate(all="ignore"):
        return (x.astype(f64) * (1.0 / d.astype(f64))).astype(f32)


def subnormal(q):
    return (q != 0) & (np.abs(q) < TINY)


def f16_boundaries():
    """Every finite f16 value h of both signs as f32, the midpoint of h and its successor (exact in f32; 65520 after 65504), the f32
    neighbours one ulp either side of each, 65520 / 2^-25 / 2^-24 with their neighbours, f32 subnormals, +-inf and NaN."""
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(f64)
    succ = np.concatenate([h[1:], [65536.0]])
    mid = (h + succ) / 2
    assert (mid.astype(f32).astype(f64) == mid).all() and mid[-1] == 65520.0 and mid[0] == 2.0 ** -25
    base = np.concatenate([h, mid]).astype(f32)
    x = np.concatenate([around(base, 1), around(np.array([65520.0, 2.0 ** -25, 2.0 ** -24], dtype=f32), 3),
                        from_bits(np.array([1, 2, 0x400000, 0x7FFFFF, 0x800000], dtype=u32)), np.array([np.inf, np.nan], dtype=f32)])
    return np.concatenate([x, -x])


def numpy_f16_roundtrip(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(f32)


def f16_product_ties(seed=106, n=400_000):
    """Pairs whose exact product lies within half an f32 ulp of an f16 tie t without being t: RN32(a b) = t, so two roundings go to
    the even neighbour of t while one rounding goes to the side the product is on.  Only the pairs where those differ are kept (the
    construction, checked in f64 where a 24 x 24-bit product is exact), with both signs, and pairs with a b = -0."""
    rng = np.random.default_rng(seed)
    hb = rng.integers(1, 0x7BFF, n, dtype=np.uint16)
    h = hb.view(np.float16).astype(f64)
    t = (h + (hb + np.uint16(1)).view(np.float16).astype(f64)) / 2
    a = rng.uniform(1.0, 2.0, n).astype(f32)
    b = (t / a.astype(f64)).astype(f32)
    p = a.astype(f64) * b.astype(f64)
    keep = (p.astype(f32).astype(f64) == t) & (p != t)
    a, b, p = a[keep], b[keep], p[keep]
    once, twice = p.astype(np.float16), p.astype(f32).astype(np.float16)
    differ = once != twice
    a, b = a[differ], b[differ]
    assert a.size > n // 8, a.size
    a, b = np.concatenate([a, -a, a]), np.concatenate([b, b, -b])
    p = a.astype(f64) * b.astype(f64)
    assert (p.astype(np.float16) != p.astype(f32).astype(np.float16)).all()  # one and two roundings really differ, everywhere
    za = np.array([-0.0, 0.0, -1e-30, 1e-30, -1e-45, 1e-45, -0.0, 3.0], dtype=f32)
    zb = np.array([1.0, -1.0, 1e-30, -1e-30, 1e-45, -0.5, 0.0, -0.0], dtype=f32)
    assert (bits(za * zb) == 0x80000000).all()
    return np.concatenate([a, za]), np.concatenate([b, zb])


def norm_encoder_inputs(scale, lo_code, hi_code):
    """Every code's lower and upper tie point (k +- 0.5) / scale with two f32 neighbours either side, values below and above the
    clamp range, +-0, +-inf, NaN (the clamp drops it to the low bound), and the whole unary domain."""
    k = np.arange(lo_code, hi_code + 1, dtype=f64)
    ties = np.concatenate([(k - 0.5) / scale, (k + 0.5) / scale, k / scale]).astype(f32)
    extra = np.array([-1.5, -1.0, 1.0, 1.5, 2.0, -2.0, 1e30, -1e30, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45], dtype=f32)
    return np.concatenate([around(ties, 2), around(extra[np.isfinite(extra)], 2), extra, unary_domain(500)])


def shading_inputs(seed=0, n=200_000):
    """Ops 11..13 and 16..19 (the inputs of the former printing script tests/tools/probe_shading.py): scalar clamps, then V N L base colour radiance
    + roughness for shading() / env_brdf(), with grazing N.L / N.V, the roughness clamp, zero vectors and radiance up to f16 max."""
    rng = np.random.default_rng(seed)
    sx = np.concatenate([np.array([-0.0, 0.0, -1e-30, 1e-30, np.nan, -np.inf, np.inf, 1.0, -1.0, 2.0, -2.0], f32), rng.normal(0, 1, 1000).astype(f32),
                         around(np.array([0.0, 1.0, -1.0], dtype=f32), 4)])
    sy = np.concatenate([np.array([1.0, 1.0, 1, 1, 1, 1, 1, 1, 1, 1, -0.0], f32), rng.normal(0, 1, 1000).astype(f32), np.ones(27, f32)])
    x = rng.normal(0, 1, (n, 16)).astype(f32)
    x[:, 9:12] = rng.uniform(0, 1, (n, 3))
    x[:, 12:15] = rng.uniform(0, 300, (n, 3))
    x[:, 15] = rng.choice([0.0, 1.0, 2.0], n)
    x[:, 6:9] = x[:, 3:6] + 0.8 * x[:, 6:9]  # N.L and N.V mostly positive
    x[:, 0:3] = x[:, 3:6] + 0.8 * x[:, 0:3]
    y = rng.choice([1.0, 0.5, 0.089, 0.3], n).astype(f32)
    # grazing: N = +z, L and V in the xy plane lifted by a z within a few ulp of 0 either side (and exactly 0)
    z = np.concatenate([around(np.array([0.0], dtype=f32), 4), np.array([1e-38, -1e-38, 1e-20, -1e-20, 6e-8, -6e-8, 1.2e-7, -1.2e-7, 1e-4, -1e-4], dtype=f32)])
    g = n // 4
    phi = rng.uniform(0, 2 * np.pi, (2, g))
    x[:g, 3:6] = [0.0, 0.0, 1.0]
    x[:g, 6], x[:g, 7], x[:g, 8] = np.cos(phi[0]), np.sin(phi[0]), rng.choice(z, g)
    x[:g, 0], x[:g, 1], x[:g, 2] = np.cos(phi[1]), np.sin(phi[1]), rng.choice(z, g)
    x[: g // 2, 2] = rng.uniform(0.1, 1.0, g // 2)  # half of them graze with the light alone
    # every roughness the clamp at 0.089 touches: the threshold's neighbours, below it, zero, above one, NaN
    rough = np.concatenate([around(np.array([0.089], dtype=f32), 64), around(np.array([1.0], dtype=f32), 8), np.array([0.0, -0.0, 0.01, 0.05, 0.0889, 1.5, -1.0, np.nan], f32)])
    y[g : 2 * g] = rng.choice(rough, g)
    y[g : g + rough.size] = rough
    # zero vectors: normalize gives NaN on both sides
    for j, c in enumerate((0, 3, 6)):
        x[2 * g + j : 2 * g + 300 : 3, c : c + 3] = 0.0
    x[2 * g + 300 : 2 * g + 400, 12:15] = rng.choice([65504.0, 60000.0, 32768.0, 0.0], (100, 3))  # radiance up to the f16 maximum
    x[2 * g + 400 : 3 * g, 12:15] = rng.uniform(0, 65504.0, (g - 400, 3))
    return (sx, sy), (np.ascontiguousarray(x), y)


def vector_inputs(seed=107, n=200_000):
    """16 floats per item (and 4 of y for the 4x4 product) in which x and y terms nearly cancel, so that every rounding of the
    chain shows: v random, rows (s v.y', -s v.x, c, ..) with v.y' a few ulp from v.y - the sum of the first two products is of the
    order of their rounding error, the third term of the same order.  A share of plain random, huge, tiny and zero vectors is mixed in."""
    rng = np.random.default_rng(seed)
    r = lambda *shape: (rng.normal(0, 1, shape) * np.exp(rng.uniform(-3, 3, shape))).astype(f32)
    jit = lambda a: from_bits((bits(a).astype(np.int64) + rng.integers(-3, 4, a.shape)).astype(u32))
    out = {}
    v = r(n, 4)
    row = np.empty((n, 4), f32)
    s, s2 = r(n), r(n)
    row[:, 0], row[:, 1] = s * jit(v[:, 1]), -s * v[:, 0]
    row[:, 2] = (np.abs(row[:, 0] * v[:, 0]) * f32(2.0 ** -23) * rng.uniform(0.2, 4, n) / np.maximum(np.abs(v[:, 2]), f32(1e-6))).astype(f32)
    row[:, 3] = (np.abs(row[:, 0] * v[:, 0]) * f32(2.0 ** -23) * rng.uniform(0.2, 4, n) / np.maximum(np.abs(v[:, 3]), f32(1e-6))).astype(f32)
    x = r(n, 16)
    x[:, 0:3], x[:, 3:6] = row[:, :3], v[:, :3]
    out["dot3"] = x.copy()
    x[:, 0:4], x[:, 4:8] = row, v
    out["dot4"] = x.copy()
    # cross: b nearly parallel to a
    a = r(n, 3)
    x = r(n, 16)
    x[:, 0:3], x[:, 3:6] = a, jit(a * r(n)[:, None])
    out["cross"] = x.copy()
    # mat3 * v: the ROWS of the matrix cancel against v; columns c0 c1 c2 = q[0..2], q[3..5], q[6..8]
    x = r(n, 16)
    y4 = v.copy()
    m4 = np.empty((n, 4, 4), f32)  # [column, row]
    for i in range(4):
        si = r(n)
        m4[:, 0, i], m4[:, 1, i] = si * jit(v[:, 1]), -si * v[:, 0]
        scale = np.abs(m4[:, 0, i] * v[:, 0]) * f32(2.0 ** -23)
        m4[:, 2, i] = (scale * rng.uniform(0.2, 4, n) / np.maximum(np.abs(v[:, 2]), f32(1e-6))).astype(f32)
        m4[:, 3, i] = (scale * rng.uniform(0.2, 4, n) / np.maximum(np.abs(v[:, 3]), f32(1e-6))).astype(f32)
    x[:, 0:9] = m4[:, :3, :3].reshape(n, 9)
    x[:, 9:12] = v[:, :3]
    out["mul3"] = x.copy()
    out["mul4"] = (m4.reshape(n, 16).copy(), y4)
    # normalize / length: every scale, overflow and underflow of dot(a, a), the zero vector
    x = r(n, 16)
    x[:, 0:3] *= np.exp(rng.uniform(-60, 60, n)).astype(f32)[:, None]
    x[:64, 0:3] = 0.0
    x[64:128, 0:3] = [-0.0, 0.0, -0.0]
    x[128:192, 0:3] = rng.choice(np.array([1e-45, 1e-38, 3e38, np.inf, np.nan, 0.0], dtype=f32), (64, 3))
    out["normalize"] = x.copy()
    # mix(a, b, t) = a (1 - t) + b t
    x = r(n, 16)
    x[:, 2] = rng.uniform(-0.5, 1.5, n)
    x[: n // 4, 1] = -x[: n // 4, 0] * (1 - x[: n // 4, 2]) / np.where(x[: n // 4, 2] == 0, f32(1), x[: n // 4, 2])
    x[:8, 2] = [0.0, 1.0, -0.0, np.nan, np.inf, 0.5, 1e-45, 2.0]
    out["mix"] = x.copy()
    u = unary_domain(100, seed=seed)
    x = r(u.size, 16)
    x[:, 0] = u
    out["fract"] = x
    for k in ("dot3", "dot4", "cross", "mul3"):
        out[k][:256, :12] = r(256, 12) * np.exp(rng.uniform(-80, 80, (256, 1))).astype(f32)  # huge and tiny: overflow and subnormals in the chain
    return out


def fma32(a, b, c):
    """fmaf in numpy, exactly: the f64 product p of two f32 numbers is exact; TwoSum gives s = RN64(p + c) and its exact error e;
    where e != 0 the sum lies strictly between s and its f64 neighbour on e's side, and the one of those two with an odd mantissa
    is the sum rounded to odd - which rounds to f32 (29 bits fewer) the way the exact sum does.  No double rounding."""
    a, b, c = (np.asarray(v, dtype=f32).astype(f64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        fix = np.isfinite(s) & (e != 0) & (s.view(np.int64) & 1 == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


# -------------------------------------------------------------------------------------------------------------- CPU: the oracle
def test_oracle_sin_cos_accuracy_where_the_reduction_cancels():
    """The file's 2.5e-7 absolute bound, on the [-10, 10] sample plus the 64 f32 neighbours either side of k pi/2, k = 0..8, where
    the two-term Cody-Waite reduction cancels.  Measured: max |error| 8.3e-8 (sin) / 8.9e-8 (cos) over the set, 1.9e-9 on the
    neighbours of k pi/2 alone."""
    rng = np.random.default_rng(1)
    near = np.concatenate([around(np.array([k * np.pi / 2], dtype=f32), 64) for k in range(9)])
    near = np.concatenate([near, -near])
    x = np.concatenate([rng.uniform(-10.0, 10.0, 100_000).astype(f32), near])
    es, ec = np.abs(orc(0, x) - np.sin(x.astype(f64))), np.abs(orc(1, x) - np.cos(x.astype(f64)))
    print(f"max |sin_ - sin| = {es.max():.3e} ({es[-near.size:].max():.3e} near k pi/2), max |cos_ - cos| = {ec.max():.3e} ({ec[-near.size:].max():.3e} near k pi/2)")
    assert es.max() < 2.5e-7
    assert ec.max() < 2.5e-7


def test_oracle_f16_roundtrip_matches_numpy_at_every_boundary():
    x = f16_boundaries()
    assert_same(orc(8, x), numpy_f16_roundtrip(x), "oracle f16 vs numpy.float16", (x,))


def test_oracle_div_sqrt_are_ieee_at_the_edges():
    for a, b in (division_edges(), binary_domain()):
        with np.errstate(all="ignore"):
            want = a / b
        assert_same(orc(9, a, b), want, "oracle a / b vs numpy float32", (a, b))
    s = np.concatenate([unary_domain(), np.array([-0.0, 0.0, -1.0, -1e-45, 1e-45, np.inf, -np.inf, np.nan], dtype=f32)])
    with np.errstate(all="ignore"):
        want = np.sqrt(s)
    assert_same(orc(10, s), want, "oracle sqrtf vs numpy float32", (s,))
    assert bits(orc(10, np.array([-0.0], f32)))[0] == 0x80000000


def test_quotient_by_reciprocal_proof_in_numpy():
    """hk_device_math.hpp's argument for quotient_by_reciprocal, checked: RN32(f64(x) * (1 / f64(d))) IS the IEEE quotient wherever
    that quotient is normal or zero (or infinite or NaN), for every pair - adversarial numerators on rounding boundaries of the
    normal and of the subnormal grid included.  They differ only where the IEEE quotient is subnormal (a tie of the subnormal grid
    is hit exactly and the reciprocal's error decides it), and there exp_ of both values is exactly 1.0f - the property the denoiser
    relies on.  Measured: 180 252 of 10 959 114 pairs differ, all of them with a subnormal IEEE quotient."""
    x, d = quotient_pairs()
    with np.errstate(all="ignore"):
        ieee = x / d
    emul = reciprocal_emulation(x, d)
    sub = subnormal(ieee)
    differ = (bits(ieee) != bits(emul)) & ~(np.isnan(ieee) & np.isnan(emul))
    print(f"{differ.sum()} of {x.size} pairs differ, {(differ & sub).sum()} with a subnormal IEEE quotient, {(differ & (ieee == 0)).sum()} with a zero one; "
          f"{sub.sum()} subnormal quotients, {((ieee == 0) & (x != 0) & np.isfinite(d)).sum()} that round to zero")
    assert_same(emul[~sub], ieee[~sub], "reciprocal emulation vs IEEE where the quotient is normal or zero", (x[~sub], d[~sub]))
    assert not (differ & ~sub).any()
    assert (differ & sub).sum() > 1000, "the pairs must reach subnormal quotients where the two differ"
    assert ((ieee == 0) & (x != 0) & np.isfinite(d)).sum() > 1000, "the pairs must reach quotients that round to zero"
    assert (np.abs(emul[differ]) < TINY).all()
    for v in (ieee[differ], emul[differ], ieee[sub], emul[sub]):
        assert (bits(orc(2, v)) == 0x3F800000).all(), "exp_ of a subnormal quotient (and of what the reciprocal makes of it) must be exactly 1.0f"


def test_oracle_sin_cos_are_pure_for_huge_and_special_arguments():
    """After reduce_pio2 converts its quadrant with the saturating i32(): the result depends on the argument's bits alone."""
    u = unary_domain(500)
    x = np.concatenate([u[~(np.abs(u) < 1e9)], np.array([3.4e9, -3.4e9, 2147483648.0 * 1.6, 1e10, -1e10, 3e38, -3e38], dtype=f32)])
    assert np.isnan(x).any() and np.isinf(x).any() and (np.abs(x[np.isfinite(x)]) > 3.4e9).sum() > 10_000
    perm = np.random.default_rng(5).permutation(x.size)
    for op in (0, 1):
        first, second, moved = orc(op, x), orc(op, x), orc(op, x[perm])
        assert (bits(first) == bits(second)).all()
        assert (bits(first[perm]) == bits(moved)).all()
        padded = orc(op, np.concatenate([np.zeros(3, f32), x]))[3:]  # another position, another alignment of any vectorised loop
        assert (bits(first) == bits(padded)).all()
        assert np.isnan(first[~np.isfinite(x)]).all()
    # the quadrant of a saturated conversion is INT_MAX & 3 = 3 (-cos_poly / sin_poly), not INT_MIN & 3 = 0
    big = np.array([1e10, 3e38], dtype=f32)
    kf = np.floor(fma32(big, np.full(2, 0.63661977236758134308, f32), np.full(2, 0.5, f32)))
    assert (kf > 2.0 ** 31).all()
    r = fma32(kf, np.full(2, 4.37113882867379e-8, f32), fma32(kf, np.full(2, -1.57079637050628662109375, f32), big))
    assert np.isfinite(r).all()
    with np.errstate(over="ignore"):  # (the reduced argument of 3e38 is huge itself: the polynomial overflows, on both sides alike)
        z = (r * r).astype(f32)
        p = fma32(fma32(np.full(2, 2.443315711809948e-5, f32), z, np.full(2, -1.388731625493765e-3, f32)), z, np.full(2, 4.166664568298827e-2, f32))
        cos_poly = fma32((p * z).astype(f32), z, fma32(np.full(2, -0.5, f32), z, np.ones(2, f32)))
    assert_same(orc(0, big), -cos_poly, "sin_ of a saturated quadrant", (big,))


def test_vector_inputs_tell_contracted_from_contract_order():
    """In float64: on the cancelling sets the contract's fma chain differs from the same sum evaluated unfused, and from the chain
    with its x and z terms swapped, for at least HALF of the items (the sum of the first two products is of the order of one rounding
    error, so every rounding shows; measured 0.999) - so a build without -ffp-contract=off or with a reordered chain cannot pass.
    mix(a, b, t) is written unfused; its contraction fma(b, t, a (1 - t)) differs for at least a tenth of its set."""
    with np.errstate(all="ignore"):  # (the huge and tiny rows overflow and underflow on purpose)
        shares = _order_shares(vector_inputs())
    print(shares)
    for k, s in shares.items():
        assert s >= (0.1 if k.startswith("mix") else 0.5), (k, s)


def _order_shares(d):
    q = d["dot3"]
    a, b = q[:, 0:3], q[:, 3:6]
    chain = fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))
    assert_same(orc(NEW["dot3"], q)[256:], chain[256:], "numpy's model of the contract's dot", (q[256:, 0],))
    unfused = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    swapped = fma32(a[:, 0], b[:, 0], fma32(a[:, 1], b[:, 1], a[:, 2] * b[:, 2]))
    shares = {"dot3 unfused": (chain != unfused).mean(), "dot3 swapped": (chain != swapped).mean()}
    q = d["dot4"]
    a, b = q[:, 0:4], q[:, 4:8]
    chain = fma32(a[:, 3], b[:, 3], fma32(a[:, 2], b[:, 2], fma32(a[:, 1], b[:, 1], a[:, 0] * b[:, 0])))
    shares["dot4 unfused"] = (chain != ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) + a[:, 3] * b[:, 3]).mean()
    q = d["cross"]
    a, b = q[:, 0:3], q[:, 3:6]
    shares["cross.x unfused"] = (fma32(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])) != a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]).mean()
    shares["cross.x swapped"] = (fma32(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])) != -fma32(a[:, 2], b[:, 1], -(a[:, 1] * b[:, 2]))).mean()
    q = d["mul3"]
    v = q[:, 9:12]
    chain = fma32(q[:, 6], v[:, 2], fma32(q[:, 3], v[:, 1], q[:, 0] * v[:, 0]))
    shares["mul3.x unfused"] = (chain != (q[:, 0] * v[:, 0] + q[:, 3] * v[:, 1]) + q[:, 6] * v[:, 2]).mean()
    m, v = d["mul4"]
    chain = fma32(m[:, 12], v[:, 3], fma32(m[:, 8], v[:, 2], fma32(m[:, 4], v[:, 1], m[:, 0] * v[:, 0])))
    shares["mul4.x unfused"] = (chain != ((m[:, 0] * v[:, 0] + m[:, 4] * v[:, 1]) + m[:, 8] * v[:, 2]) + m[:, 12] * v[:, 3]).mean()
    q = d["mix"]
    a, b, t = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        shares["mix contracted"] = (fma32(b, t, a * (f32(1.0) - t)) != a * (f32(1.0) - t) + b * t).mean()
    return shares


# ------------------------------------------------------------------------------------------- GPU: device against oracle, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("op", [k for k in OPS if k != "f16"])
def test_device_ops_0_to_10_over_the_domain(eng, op):
    if op in ("pow", "min", "max", "div"):
        args = binary_domain()
        if op == "div":
            e = division_edges()
            args = (np.concatenate([args[0], e[0]]), np.concatenate([args[1], e[1]]))
    else:
        args = (unary_domain(),)
    assert_same(eng.debug_math(OPS[op], *args), orc(OPS[op], *args), op, args)


@pytest.mark.gpu
def test_device_f16_boundaries_three_way(eng):
    x = f16_boundaries()
    got, want, ref = eng.debug_math(8, x), orc(8, x), numpy_f16_roundtrip(x)
    assert_same(got, want, "device f16 vs oracle", (x,))
    assert_same(got, ref, "device f16 vs numpy.float16", (x,))
    assert_same(want, ref, "oracle f16 vs numpy.float16", (x,))
    u = unary_domain()
    assert_same(eng.debug_math(8, u), orc(8, u), "device f16 vs oracle over the domain", (u,))


@pytest.mark.gpu
def test_device_f16_of_a_product_rounds_twice(eng):
    """f16(a * b) is RN16(RN32(a b)): the barrier in f32_to_f16 keeps the product out of v_fma_mixlo_f16 (one rounding, -0 -> +0)."""
    a, b = f16_product_ties()
    got = eng.debug_math(NEW["f16_product"], a, b)
    assert_same(got, orc(NEW["f16_product"], a, b), "device f16(a*b) vs oracle", (a, b))
    assert_same(got, numpy_f16_roundtrip(a * b), "device f16(a*b) vs numpy's two roundings", (a, b))
    a, b = binary_domain()
    assert_same(eng.debug_math(NEW["f16_product"], a, b), orc(NEW["f16_product"], a, b), "device f16(a*b) vs oracle over the domain", (a, b))


@pytest.mark.gpu
def test_device_sincos_is_sin_and_cos(eng):
    x = unary_domain()
    for new, old, name in ((NEW["sincos_sin"], 0, "sin"), (NEW["sincos_cos"], 1, "cos")):
        got = eng.debug_math(new, x)
        assert_same(got, orc(old, x), f"sincos_ {name} vs the oracle's {name}_", (x,))
        assert_same(got, eng.debug_math(old, x), f"sincos_ {name} vs the device's own {name}_", (x,))


@pytest.mark.gpu
def test_device_exp_nonpositive_is_exp(eng):
    u = unary_domain()
    e = edge_inputs("exp", np.random.default_rng(11))[0]
    x = np.concatenate([u[(bits(u) >> 31 == 1) | (u == 0)], e[~(e > 0)], np.array([-0.0, 0.0, np.nan, -np.nan], dtype=f32)])
    assert (bits(x) == 0x80000000).any() and np.isnan(x).any() and ((x < -85) & (x > -104.5)).sum() > 100_000
    assert_same(eng.debug_math(NEW["exp_nonpositive"], x), orc(OPS["exp"], x), "exp_nonpositive_ vs exp_", (x,))


@pytest.mark.gpu
def test_device_quotient_by_reciprocal(eng):
    """The IEEE quotient wherever it is normal or zero (test_quotient_by_reciprocal_proof_in_numpy), the numpy emulation everywhere."""
    x, d = quotient_pairs()
    got = eng.debug_math(NEW["quotient"], x, d)
    ok = ~subnormal(orc(OPS["div"], x, d))
    assert_same(got[ok], orc(OPS["div"], x[ok], d[ok]), "quotient_by_reciprocal vs a / b", (x[ok], d[ok]))
    assert_same(got, reciprocal_emulation(x, d), "quotient_by_reciprocal vs its numpy emulation", (x, d))


@pytest.mark.gpu
def test_device_denoise_weight_is_exp_of_the_ieee_quotient(eng):
    """exp_nonpositive_(quotient_by_reciprocal(-|a|, 1 / b)) == exp_((-|a|) / b) with no exceptions."""
    for name, (a, b) in (("the denoiser's domain", denoise_domain()), ("the binary domain, b > 0", binary_domain()), ("the division edges, b > 0", division_edges()),
                           ("the boundary numerators, b > 0", reciprocal_adversaries())):
        keep = b > 0 if name != "the denoiser's domain" else np.ones(b.size, bool)
        a, b = a[keep], b[keep]
        want = orc(NEW["denoise_weight"], a, b)
        with np.errstate(all="ignore"):
            assert_same(want, orc(OPS["exp"], -np.abs(a) / b), "the oracle's weight vs exp_ of numpy's quotient", (a, b))
        assert_same(eng.debug_math(NEW["denoise_weight"], a, b), want, f"denoise weight over {name}", (a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pow2", "pow5", "pow16", "pow_quarter"])
def test_device_constant_powers(eng, name):
    rng = np.random.default_rng(12)
    u = unary_domain()
    h = np.arange(0x3C01, dtype=np.uint16).view(np.float16).astype(f32)  # the f16 grid of [0, 1]
    x = np.concatenate([rng.uniform(0, 1, 1_000_000).astype(f32), np.exp(rng.uniform(-104, 0, 500_000)).astype(f32), around(np.array([0.0, 1.0, 0.5], f32), 64), h,
                        u[bits(u) >> 31 == 0]])
    want = orc(NEW[name], x)
    assert_same(eng.debug_math(NEW[name], x), want, name, (x,))
    if name != "pow_quarter":
        assert np.isinf(want).any() and ((want != 0) & (np.abs(want) < TINY)).any() and ((want == 0) & (x != 0)).any()  # overflow, subnormal, underflow


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale,lo,hi", [("unorm16", 65535.0, 0, 65535), ("snorm8", 127.0, -127, 127)])
def test_device_norm_encoders_at_their_ties(eng, name, scale, lo, hi):
    x = norm_encoder_inputs(scale, lo, hi)
    want = orc(NEW[name], x)
    assert_same(eng.debug_math(NEW[name], x), want, name, (x,), nan_equal=False)
    assert np.unique(want).size == hi - lo + 1  # every code is reached
    nan = orc(NEW[name], np.array([np.nan], f32))[0]
    assert nan == (0.0 if name == "unorm16" else 129.0)  # the clamp drops NaN to its low bound: code 0, or -127 & 0xff


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["to_u32", "to_i32"])
def test_device_saturating_conversions(eng, name):
    x = np.concatenate([unary_domain(), around(np.array([2.0 ** 31, 2.0 ** 32, -(2.0 ** 31), -(2.0 ** 32), 0.0, 1.0, -1.0, 2.0 ** 24], dtype=f32), 8),
                        np.array([np.nan, np.inf, -np.inf], dtype=f32)])
    want = orc(NEW[name], x)
    assert_same(eng.debug_math(NEW[name], x), want, name, (x,), nan_equal=False)  # all 32 bits are the integer
    with np.errstate(all="ignore"):
        t = np.trunc(np.where(np.isnan(x), f32(0), x).astype(f64))
    ref = np.clip(t, 0.0, 4294967295.0).astype(np.uint64).astype(u32) if name == "to_u32" else np.clip(t, -2147483648.0, 2147483647.0).astype(np.int64).astype(np.int32).view(u32)
    assert (bits(want) == ref).all()


@pytest.mark.gpu
def test_device_clamps_and_shading(eng):
    (sx, sy), (x, y) = shading_inputs()
    u = unary_domain(500)
    for op in (11, 12):
        for arg in (sx, u):
            assert_same(eng.debug_math(op, arg), orc(op, arg), f"op {op}", (arg,))
    a, b = binary_domain()
    for arg in ((sx, sy), (a, b)):
        assert_same(eng.debug_math(13, *arg), orc(13, *arg), "saturate(a * b)", arg)
    assert ((x[:, 0:3] == 0).all(axis=1).any() and (x[:, 3:6] == 0).all(axis=1).any() and (x[:, 6:9] == 0).all(axis=1).any())  # normalize(0) = NaN inside
    for op in (16, 17, 18, 19):
        assert_same(eng.debug_math(op, x, y), orc(op, x, y), f"op {op} (shading / env_brdf)", (x[:, 8], y))


@pytest.mark.gpu
def test_device_vector_ops_in_contract_order(eng):
    d = vector_inputs()
    for name, key in (("dot3", "dot3"), ("dot4", "dot4"), ("cross", "cross"), ("normalize", "normalize"), ("mul3", "mul3"), ("length", "normalize"), ("mix", "mix"),
                      ("fract", "fract"), ("mul4", "mul4")):
        x, y = d[key] if key == "mul4" else (d[key], None)
        for op in np.atleast_1d(NEW[name]):
            want = orc(int(op), x, y)
            assert_same(eng.debug_math(int(op), x, y), want, f"{name} (op {op})", (x[:, 0],))
        if name == "normalize":
            assert np.isnan(want[:64]).all()
