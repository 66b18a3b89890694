"""References and cases for the tile rasterisers alone (bgs_selftest_raster: raster_scan_kernel / raster_tile and raster_kernel
of csrc/render_kernels.hip on caller-supplied records and supertile lists). Pure numpy; tests/test_raster_stage_host.py
shows on the CPU what each case holds, tests/test_raster_stage_gpu.py compares on the device.

THE REFERENCE (`render_reference`) is a float64 renderer of the STAGE's inputs: per tile it takes the entries of the tile's
supertile list, in list order, whose packed rectangle holds the tile (limits inclusive, the first min(total, coarse_cap)
entries), reads the raw record words, and applies per pixel and per sample the formulas blend_px / blend_px_ms document:
    OBB     u = m00 dx + m01 dy, v = m10 dx + m11 dy  (dx, dy from the quad centre to the pixel centre or the sample),
            covered <=> max(|u|, |v|) <= 1, alpha = min(a exp(-4.5 (u^2 + v^2)), 0.999f) at the pixel CENTRE;
    AABB3D  u = m00 dx, v = m11 dy, power = B u v - (A u^2 + C v^2) / 2, the fragment dropped where power > 0,
            alpha = min(a exp(power), 0.999f);
    overlay max(|u|, |v|) > 1 - 2 * 0.08f at the centre: colour (0.3, 1, 0.1), alpha 1 (multisampled OBB: a fragment with
            u^2 + v^2 > 9 is dropped first);
    depth   a sample is covered only where z >= d (the record's z against the sample's depth, both binary32: exact);
    blend   while mean_s(T_s) >= t_eps:  w = alpha mean_s(cov_s T_s),  C += w c,  T_s *= 1 - alpha on covered samples;
            t_eps = min(2^-13, 2^-11 / cmax) in binary32 (frame_t_eps);
    resolve (C + M clear.rgb, M clear.a + 1 - M), M = mean_s(T_s).
    surfel  quad as AABB3D (u = m00 dx, v = m11 dy, covered <=> max(|u|, |v|) <= 1); the pixel's ray meets the surfel at
            (us, vs) = p.xy / p.z, p = pc.x A + pc.y B + C with pc = (u radius + mean.x, v radius aspect + mean.y), A, B, C the
            record's cross products and aspect = viewport_w / viewport_h in binary32;
            alpha = min(a exp(-min(us^2 + vs^2, 2 |mean - pc|^2) / 2), 0.999f); no discard;
It does not batch, knows nothing of keep / interior / strip verdicts, queues or rounds: those may only skip work that adds
nothing. It does not model surfel_negligible_in_tile: what that drops is at most 2^-23 of the record's opacity, which is added
to the bound of every surfel record's alpha (not under the overlay, where nothing is dropped). The integer reference does
model it (negligible_figure), and tests/test_raster_stage_host.py checks that promise pixel by pixel.

THE ERROR BOUND. e = 2^-24 (1 + 2^-10) per rounded binary32 operation (the factor covers second-order terms). Derived from
the operations the kernels perform, in the order they perform them:
  u (OBB)   staged as m' = C m (C = OBB_C, itself rounded: 2 e), dx0 = ox - cx (e), U0' = fma(m01', dy0, m00' dx0) (2 e), then
            u' = fma(m01', yl, fma(m00', xl, U0')) (2 e): every one of the four terms m.d carries at most 4 e of relative
            error and every one of the four sums rounds once against a partial sum no larger than the sum of the terms'
            magnitudes, so  du <= 8 e (|m00| (|dx0| + xl) + |m01| (|dy0| + yl))  — the cancellation in U0 + m00 x + m01 y
            taken from the magnitudes, not from |u|. A sample adds du_s = fma(m01', oy, m00' ox) (3 e of its magnitude) and one
            sum (e |u_s|); the limit OBB_C is rounded (e).
  u (AABB)  dx = x - cx (e), u = m00 dx (e): du <= 2 e |u|; a sample adds m00 ox (e) and a sum (e), the limit 1 is exact.
            Where every one of these operations is EXACT in binary32 (power-of-two coefficients on the sample grid) the
            reference's value is the kernel's value and the sample is decided whatever the band says.
  alpha     OBB: arg' = fma(u', u', v' v') (2 e arg'), e2 = v_exp_f32(-arg') (1 ulp = 2 e; ln2 |d arg'| through it),
            alpha = min(e2 a, 0.999f) (e):  d alpha / alpha <= 9 (|u| du + |v| dv) + 9 e (u^2 + v^2) + 3 e.
            AABB: P = |B u v| + (|A| u^2 + |C| v^2) / 2; the products and fmas of power round four times on top of the
            4 e u and v bring in (8 e P), __expf is v_exp_f32(power log2 e): one product and the rounded constant (2 e |power|)
            and 1 ulp (2 e), the product with a (e):  d alpha / alpha <= 10 e P + 3 e. The discard is undecided where
            |power| <= 8 e P.
            surfel: p's components are sums of products whose magnitudes are known (pc.x = a_x xl + (U0 radius + mean.x), ...): each
            term passes at most 9 rounded operations, dp_i <= 9 e (|A_i| m_x + |B_i| m_y + |C_i|) with m_x, m_y the summed
            magnitudes of pc; v_rcp_f32 is 1 ulp (2 e) and the quotient's product e; s3 = fma(us, us, vs vs) (2 e); the
            screen-space side cancels against |mean| (6 e of the magnitudes); min is 1-Lipschitz in the larger of the two
            errors:  d alpha / alpha <= max(d s3, d s2) / 2 + e min(s3, s2) + 3 e. Where the ray grazes the plane (p.z small
            against its terms) the bound grows as the kernel's error does.
  T, w, C   single-sampled: w = T alpha (e w), C = fma(w, c, C) (e |C|), T = T - w (e T):
                dw <= alpha dT + T d alpha + e w;  dC += |c| dw + e |C|;  dT' <= dT (1 - alpha) + T d alpha + e w + e T'.
            N samples: T_s = S r_s. A record moves S (one fma) or the covered r_s (one fma each), rb = mean r_s rides along
            (one fma, N - 1 sums): dT_s' <= dT_s (1 - alpha) + T_s d alpha + 2 e T_s on covered samples, and the carried mean
            S rb drifts from mean_s(T_s) by at most (N + 1) e M per blended record (D). w = (S rb) alpha or (S alpha / N) sum:
                dw <= d alpha X + alpha (mean_s(cov_s dT_s) + D) + (N + 2) e w,   X = mean_s(cov_s T_s).
  resolve   M = S rb (e): dM = mean_s(dT_s) + D + e M; colour fma(M, clear, C): |clear| dM + dC + e |out|; alpha
            fma(M, clear.a, 1 - M): (1 + |clear.a|) dM + e |1 - M| + e |out|.
  plus 2^-120 absolute for results the hardware flushes to zero.
The assertion allows TWICE the figure (the margin the vertex-stage pin took for its power function).

UNDECIDED. A sample whose |u_s| or |v_s| is within its bound of the limit, a fragment whose AABB power is within its bound of 0
or whose overlay decision is within the bound of u of 0.84, and a pixel whose M comes within dM of t_eps before a record,
make the PIXEL undecided: it is left out of the float64 comparison (never out of the bit comparison). Depth compares two
binary32 values without arithmetic and is always decided. Designed cases hold no undecided pixel, random ones at most 0.5 %.
"""
from dataclasses import dataclass, field

import numpy as np

TILE = 16
E = 2.0 ** -24 * (1.0 + 2.0 ** -10)
RECT_EMPTY = 0x000000FF
OBB, AABB3D, SURFEL = 0, 1, 2
ALPHA_MAX = float(np.float32(0.999))
BBOX_EDGE = float(np.float32(1.0) - np.float32(2.0) * np.float32(0.08))
SAMPLE_OFFSETS = {1: [(0.0, 0.0)], 2: [(0.25, 0.25), (-0.25, -0.25)],
                  4: [(-0.125, -0.375), (0.375, -0.125), (-0.375, 0.125), (0.125, 0.375)],
                  8: [(k / 16.0, l / 16.0) for k, l in ((1, -3), (-1, 3), (5, 1), (-3, -5), (-5, 5), (-7, -1), (3, 7), (7, -7))]}
PRIMARIES = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0], [1.0, 0.0, 1.0]], np.float32)
BRIGHT = (4.0, 4.0, 4.0)   # what must never be drawn


def rect(x0, x1, y0, y1):
    return np.uint32(x0 | (x1 << 8) | (y0 << 16) | (y1 << 24))


def float_bits(x):
    return int(np.float32(x).view(np.uint32))


def t_eps_of(color_max_bits):
    """frame_t_eps: min(2^-13, 2^-11 / cmax) in binary32."""
    cmax = np.uint32(color_max_bits).view(np.float32)
    with np.errstate(all="ignore"):
        return float(np.minimum(np.float32(2.0 ** -13), np.float32(2.0 ** -11) / cmax))


def obb_record(cx, cy, hx, hy, angle=0.0, rgb=(1.0, 1.0, 1.0), a=0.5, z=0.5):
    """A Record of an oriented quad with half extents (hx, hy) px turned by `angle`: uv = M (pixel - centre)."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([cx, cy, c / hx, s / hx, -s / hy, c / hy, 0.0, rgb[0], rgb[1], rgb[2], a, z], np.float32)


def aabb_record(cx, cy, m00, m11, A=1.0, B=0.0, C=1.0, rgb=(1.0, 1.0, 1.0), a=0.5, z=0.5):
    return np.array([cx, cy, m00, m11, A, B, C, rgb[0], rgb[1], rgb[2], a, z], np.float32)


@dataclass
class Case:
    name: str
    width: int
    height: int
    records: np.ndarray                 # float32 [n, 12] (or [n, 24] surfel)
    lists: np.ndarray                   # uint32 [supertiles, cap, 2]
    totals: np.ndarray                  # uint32 [supertiles]
    sup_edge: int = 32
    samples: int = 1
    variant: int = OBB
    overlay: int = 0
    modes: tuple = (0,)
    clear: tuple = (0.125, 0.25, 0.5, 0.75)
    color_max_bits: int = float_bits(1.0)
    depth: np.ndarray = None            # float32 [h, w, samples]
    heavy_tiles: tuple = ()             # run again (modes 1, 2) with these tiles in the heavy list
    viewport: tuple = None              # (viewport_w, viewport_h) of the surfel aspect; None: the target's size
    random: bool = False                # a random case: at most 0.5 % undecided pixels (designed: none)
    notes: dict = field(default_factory=dict)   # what the case is named for (test_raster_stage_host.py checks it)

    def __post_init__(self):
        if self.viewport is None:
            self.viewport = (float(self.width), float(self.height))

    @property
    def tiles_x(self):
        return -(-self.width // TILE)

    @property
    def tiles_y(self):
        return -(-self.height // TILE)

    @property
    def sup_x(self):
        return -(-self.tiles_x // self.sup_edge)

    @property
    def cap(self):
        return self.lists.shape[1]

    def t_eps(self):
        return t_eps_of(self.color_max_bits)

    def tile_entries(self, tx, ty):
        """Positions (in its supertile's list) and ranks of the tile's records, in list order."""
        s = (ty // self.sup_edge) * self.sup_x + tx // self.sup_edge
        n = min(int(self.totals[s]), self.cap)
        r = self.lists[s, :n, 1]
        hit = (tx >= (r & 255)) & (tx <= ((r >> 8) & 255)) & (ty >= ((r >> 16) & 255)) & (ty <= (r >> 24))
        pos = np.nonzero(hit)[0]
        return pos, self.lists[s, pos, 0]

    def group_hits(self, tx, ty):
        """Hits per group of 64 candidates of the tile's list: what the scan rasteriser's queue sees."""
        s = (ty // self.sup_edge) * self.sup_x + tx // self.sup_edge
        n = min(int(self.totals[s]), self.cap)
        pos, _ = self.tile_entries(tx, ty)
        return [int(((pos >= g) & (pos < g + 64)).sum()) for g in range(0, n, 64)]


def make_lists(per_list, cap=None, pad_rank=0):
    """lists / totals from a list of [(rank, rect), ...] per supertile. Unused entries hold (pad_rank, full-screen rect): a
    kernel that read them would draw them."""
    cap = cap or max(1, max(len(l) for l in per_list))
    lists = np.zeros((len(per_list), cap, 2), np.uint32)
    lists[:, :, 0] = pad_rank
    lists[:, :, 1] = rect(0, 255, 0, 255)
    totals = np.zeros(len(per_list), np.uint32)
    for s, l in enumerate(per_list):
        totals[s] = len(l)
        for i, (rank, rc) in enumerate(l[:cap]):
            lists[s, i] = (rank, rc)
    return lists, totals


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference with its carried bound
# ---------------------------------------------------------------------------------------------------------------------
def _exact32(*pairs):
    """True where every (float64 result, operands' binary32 result) pair agrees: the binary32 operation was exact."""
    ok = True
    for r64, r32 in pairs:
        ok = ok & (r64 == r32.astype(np.float64))
    return ok


def _record_terms(case, rec, tx, ty, xs, ys):
    """For one record over the tile's pixel centres (xs, ys: float64 grids): alpha, its bound, per-sample coverage, whether a
    sample / the fragment is undecided, the fragment's colour and alpha after the overlay."""
    S = case.samples
    offs = SAMPLE_OFFSETS[S]
    f = rec.astype(np.float64)
    cx, cy, a = f[0], f[1], f[19 if case.variant == SURFEL else 10]
    dx, dy = xs - cx, ys - cy
    xl, yl = xs - (tx * TILE + 0.5), ys - (ty * TILE + 0.5)
    und = np.zeros(xs.shape, bool)
    cov = np.zeros(xs.shape + (S,), bool)
    with np.errstate(all="ignore"):
        if case.variant == OBB:
            m00, m01, m10, m11 = f[2], f[3], f[4], f[5]
            dx0, dy0 = (tx * TILE + 0.5) - cx, (ty * TILE + 0.5) - cy
            u, v = m00 * dx + m01 * dy, m10 * dx + m11 * dy
            bu = 8 * E * (abs(m00) * (abs(dx0) + xl) + abs(m01) * (abs(dy0) + yl))
            bv = 8 * E * (abs(m10) * (abs(dx0) + xl) + abs(m11) * (abs(dy0) + yl))
            for k, (ox, oy) in enumerate(offs):
                us, vs = u + (m00 * ox + m01 * oy), v + (m10 * ox + m11 * oy)
                bus = bu + 3 * E * (abs(m00 * ox) + abs(m01 * oy)) + E * (np.abs(us) + 1.0)
                bvs = bv + 3 * E * (abs(m10 * ox) + abs(m11 * oy)) + E * (np.abs(vs) + 1.0)
                cov[..., k] = (np.abs(us) <= 1.0) & (np.abs(vs) <= 1.0)
                # a sample is undecided when the axis that decides it is inside its band (the other axis well inside or outside)
                near_u, near_v = np.abs(np.abs(us) - 1.0) <= bus, np.abs(np.abs(vs) - 1.0) <= bvs
                und |= (near_u & (np.abs(vs) <= 1.0 + bvs)) | (near_v & (np.abs(us) <= 1.0 + bus))
            q = u * u + v * v
            alpha_raw = a * np.exp(-4.5 * q)
            ra = 9.0 * (np.abs(u) * bu + np.abs(v) * bv) + 9.0 * E * q + 3.0 * E
            frag = np.ones(xs.shape, bool)
            if case.overlay and S > 1:
                frag = ~(q > 9.0)
        elif case.variant == SURFEL:
            # record: cx cy m00 m11 | radius mean.x mean.y | A = T1 x T2 | B = T2 x T0 | C = T0 x T1 | r g b a | z
            m00, m11, radius, mx, my = f[2], f[3], f[4], f[5], f[6]
            Av, Bv, Cv = f[7:10], f[10:13], f[13:16]
            aspect = float(np.float32(case.viewport[0]) / np.float32(case.viewport[1]))
            dx0, dy0 = (tx * TILE + 0.5) - cx, (ty * TILE + 0.5) - cy
            u, v = m00 * dx, m11 * dy
            # staged as U0 = m00 dx0 (2 e), u = fma(du, xl, U0) (e): the cancellation from the magnitudes of the two terms
            bu = 3 * E * abs(m00) * (abs(dx0) + xl)
            bv = 3 * E * abs(m11) * (abs(dy0) + yl)
            for k, (ox, oy) in enumerate(offs):
                us, vs = u + m00 * ox, v + m11 * oy
                bus = bu + E * abs(m00 * ox) + 2 * E * (np.abs(us) + 1.0)
                bvs = bv + E * abs(m11 * oy) + 2 * E * (np.abs(vs) + 1.0)
                cov[..., k] = (np.abs(us) <= 1.0) & (np.abs(vs) <= 1.0)
                near_u, near_v = np.abs(np.abs(us) - 1.0) <= bus, np.abs(np.abs(vs) - 1.0) <= bvs
                und |= (near_u & (np.abs(vs) <= 1.0 + bvs)) | (near_v & (np.abs(us) <= 1.0 + bus))
            # the pixel's ray against the surfel: pc = (u radius + mean.x, v radius aspect + mean.y), p = pc.x A + pc.y B + C,
            # (us, vs) = p.xy / p.z, power = -min(us^2 + vs^2, 2 |mean - pc|^2) / 2 (a NaN side is dropped, as fminf drops it)
            ex, ey = u * radius, v * radius * aspect
            pcx, pcy = ex + mx, ey + my
            p = [Av[i] * pcx + Bv[i] * pcy + Cv[i] for i in range(3)]
            # magnitudes of what is summed on the device (pc.x = ax xl + (U0 radius + mean.x), the same for y; each term through
            # at most 9 rounded operations: aspect, dx0, U0, b, two fmas of P0, the constant, two fmas of the pixel)
            mpx = abs(m00 * radius) * (abs(dx0) + xl) + abs(mx)
            mpy = abs(m11 * radius * aspect) * (abs(dy0) + yl) + abs(my)
            dp = [9 * E * (abs(Av[i]) * mpx + abs(Bv[i]) * mpy + abs(Cv[i])) for i in range(3)]
            usr, vsr = p[0] / p[2], p[1] / p[2]
            # v_rcp_f32 (1 ulp = 2 e) and a product (e) on top of the quotient's own terms
            dus = np.abs(usr) * (dp[0] / np.abs(p[0]) + dp[2] / np.abs(p[2]) + 3 * E)
            dvs = np.abs(vsr) * (dp[1] / np.abs(p[1]) + dp[2] / np.abs(p[2]) + 3 * E)
            dus = np.where(p[0] == 0.0, dp[0] / np.abs(p[2]), dus)
            dvs = np.where(p[1] == 0.0, dp[1] / np.abs(p[2]), dvs)
            s3 = usr * usr + vsr * vsr
            ds3 = 2 * (np.abs(usr) * dus + np.abs(vsr) * dvs) + 2 * E * s3
            # the screen-space side: D = mean - pc = -(e), formed as C2 (mean - b) + (-C2 a) xl: the cancellation against |mean|
            dex, dey = 6 * E * (mpx + abs(mx)), 6 * E * (mpy + abs(my))
            s2 = 2.0 * (ex * ex + ey * ey)
            ds2 = 4 * (np.abs(ex) * dex + np.abs(ey) * dey) + 4 * E * s2
            arg = np.fmin(s3, s2)
            darg = np.where(np.isfinite(s3), np.maximum(np.where(np.isfinite(ds3), ds3, 0.0), ds2), ds2)
            alpha_raw = a * np.exp(-0.5 * arg)
            ra = 0.5 * darg + E * arg + 3.0 * E
            frag = np.ones(xs.shape, bool)
        else:
            m00, m11, A, B, C = f[2], f[3], f[4], f[5], f[6]
            u, v = m00 * dx, m11 * dy
            bu, bv = 2 * E * np.abs(u), 2 * E * np.abs(v)
            r32 = rec.astype(np.float32)
            xs32, ys32 = xs.astype(np.float32), ys.astype(np.float32)
            dx32, dy32 = xs32 - r32[0], ys32 - r32[1]
            u32, v32 = r32[2] * dx32, r32[3] * dy32
            for k, (ox, oy) in enumerate(offs):
                us, vs = u + m00 * ox, v + m11 * oy
                du32, dv32 = r32[2] * np.float32(ox), r32[3] * np.float32(oy)
                exact = _exact32((dx, dx32), (dy, dy32), (u, u32), (v, v32), (np.full(xs.shape, m00 * ox), np.full(xs.shape, du32, np.float32)),
                                 (np.full(xs.shape, m11 * oy), np.full(xs.shape, dv32, np.float32)), (us, u32 + du32), (vs, v32 + dv32))
                bus = bu + E * abs(m00 * ox) + 2 * E * (np.abs(us) + 1.0)
                bvs = bv + E * abs(m11 * oy) + 2 * E * (np.abs(vs) + 1.0)
                cov[..., k] = (np.abs(us) <= 1.0) & (np.abs(vs) <= 1.0)
                near_u, near_v = np.abs(np.abs(us) - 1.0) <= bus, np.abs(np.abs(vs) - 1.0) <= bvs
                und |= ((near_u & (np.abs(vs) <= 1.0 + bvs)) | (near_v & (np.abs(us) <= 1.0 + bus))) & ~exact
            power = B * u * v - 0.5 * (A * u * u + C * v * v)
            P = np.abs(B * u * v) + 0.5 * (np.abs(A) * u * u + np.abs(C) * v * v)
            frag = ~(power > 0.0)
            und |= (np.abs(power) <= 8 * E * P) & (P > 0.0) & cov.any(axis=-1)
            alpha_raw = a * np.exp(power)
            ra = 10.0 * E * P + 3.0 * E
        alpha = np.minimum(alpha_raw, ALPHA_MAX)
        dalpha = np.abs(alpha_raw) * ra + 2.0 ** -120
        dalpha = np.where(alpha_raw > ALPHA_MAX * (1.0 + ra), 0.0, dalpha)   # clamped with margin: the constant itself
        if case.variant == SURFEL and not case.overlay:
            # surfel_negligible_in_tile may drop the record from the tile where it is worth at most 2^-23 of its opacity there
            dalpha = dalpha + abs(a) * 2.0 ** -23
        col = np.broadcast_to(f[16:19] if case.variant == SURFEL else f[7:10], xs.shape + (3,)).copy()
        if case.overlay:
            g = np.maximum(np.abs(u), np.abs(v))
            frame = g > BBOX_EDGE
            und |= (np.abs(g - BBOX_EDGE) <= np.maximum(bu, bv) + 2 * E) & cov.any(axis=-1)
            alpha = np.where(frame, 1.0, alpha)
            dalpha = np.where(frame, 0.0, dalpha)
            col[frame] = (float(np.float32(0.3)), 1.0, float(np.float32(0.1)))
        bad = ~np.isfinite(u) | ~np.isfinite(v)   # a NaN centre covers nothing (every compare is false)
        cov[bad] = False
        und &= ~bad
        alpha = np.where(np.isfinite(alpha), alpha, 0.0)
        dalpha = np.where(np.isfinite(dalpha), dalpha, 0.0)
    cov &= frag[..., None]
    if case.depth is not None:
        z = np.float32(rec[20 if case.variant == SURFEL else 11])
        d = case.depth[ty * TILE:ty * TILE + xs.shape[0], tx * TILE:tx * TILE + xs.shape[1]]
        cov &= (z >= d)
    return alpha, dalpha, cov, und, col


def render_reference(case, trace=None, states=None):
    """(image float64 [h, w, 4], bound [h, w, 4], undecided bool [h, w]) of a case. `trace`, a dict, receives per tile the
    record position (in the tile's own sequence) after which every pixel of the tile was below the cut-off, or None.
    `states`, a dict, receives per tile one tuple per record of its sequence, taken AFTER the record: (every pixel's mean
    transmittance is below the cut-off, that verdict is decided at every pixel — no M within its bound of t_eps —, the
    smallest and the largest M of the tile)."""
    H, W, S = case.height, case.width, case.samples
    img = np.zeros((H, W, 4))
    bound = np.zeros((H, W, 4))
    undecided = np.zeros((H, W), bool)
    t_eps = case.t_eps()
    clear = np.asarray(case.clear, np.float32).astype(np.float64)
    for ty in range(case.tiles_y):
        for tx in range(case.tiles_x):
            h, w = min(TILE, H - ty * TILE), min(TILE, W - tx * TILE)
            ys, xs = np.meshgrid(ty * TILE + np.arange(h) + 0.5, tx * TILE + np.arange(w) + 0.5, indexing="ij")
            T, dT = np.ones((h, w, S)), np.zeros((h, w, S))
            C, dC = np.zeros((h, w, 3)), np.zeros((h, w, 3))
            D = np.zeros((h, w))
            und = np.zeros((h, w), bool)
            saturated_after = None
            _, ranks = case.tile_entries(tx, ty)
            for i, rank in enumerate(ranks):
                alpha, dalpha, cov, und_r, col = _record_terms(case, case.records[int(rank)], tx, ty, xs, ys)
                M = T.mean(axis=2)
                dM = dT.mean(axis=2) + D + E * M
                live = M >= t_eps
                touched = cov.any(axis=2)
                und |= touched & (np.abs(M - t_eps) <= dM)
                und |= und_r & live
                covl = cov & live[..., None]
                X = np.where(covl, T, 0.0).mean(axis=2)
                w_ = alpha * X
                dw = dalpha * X + alpha * (np.where(covl, dT, 0.0).mean(axis=2) + np.where(touched & live, D, 0.0)) + (S + 2) * E * w_
                C += w_[..., None] * col
                dC += np.abs(col) * dw[..., None] + E * np.abs(C)
                a3, da3 = alpha[..., None], dalpha[..., None]
                Tn = np.where(covl, T * (1.0 - a3), T)
                dT = np.where(covl, dT * (1.0 - a3) + T * da3 + 2.0 * E * T + E * (w_[..., None] if S == 1 else 0.0), dT)
                T = Tn
                if S > 1:
                    D = D + np.where(touched & live, (S + 1) * E * M, 0.0)
                Ma = T.mean(axis=2)
                if saturated_after is None and (Ma < t_eps).all():
                    saturated_after = i
                if states is not None:
                    dMa = dT.mean(axis=2) + D + E * Ma
                    states.setdefault((tx, ty), []).append((bool((Ma < t_eps).all()), bool((np.abs(Ma - t_eps) > dMa).all()),
                                                            float(Ma.min()), float(Ma.max())))
            if trace is not None:
                trace[(tx, ty)] = saturated_after
            M = T.mean(axis=2)
            dM = dT.mean(axis=2) + D + E * M
            sl = (slice(ty * TILE, ty * TILE + h), slice(tx * TILE, tx * TILE + w))
            img[sl][..., :3] = C + M[..., None] * clear[:3]
            img[sl][..., 3] = M * clear[3] + (1.0 - M)
            bound[sl][..., :3] = np.abs(clear[:3]) * dM[..., None] + dC + E * np.abs(img[sl][..., :3]) + 2.0 ** -120
            bound[sl][..., 3] = (1.0 + abs(clear[3])) * dM + E * np.abs(1.0 - M) + E * np.abs(img[sl][..., 3]) + 2.0 ** -120
            undecided[sl] = und
    return img, bound, undecided


# ---------------------------------------------------------------------------------------------------------------------
# the integer reference: a tile's cost word, its staging rounds and the heavy feedback
# ---------------------------------------------------------------------------------------------------------------------
def work_constants(path=None):
    """WORK_BLENDED, WORK_STAGED, WORK_ROUND, WORK_GROUP as csrc/render_kernels.hip states them."""
    import os
    import re
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bevy_gaussian_splatting_amd", "csrc", "render_kernels.hip")
    m = re.search(r"constexpr uint32_t WORK_BLENDED = (\d+)u, WORK_STAGED = (\d+)u, WORK_ROUND = (\d+)u, WORK_GROUP = (\d+)u;", open(path).read())
    return {"blended": int(m.group(1)), "staged": int(m.group(2)), "round": int(m.group(3)), "group": int(m.group(4))}


KEEP_SLACK, KEEP_MARGIN = 1.0001, 1e-5   # raster_tile's slack; how far from it a float64 figure must lie to be decided (binary32: ~1e-6)
# surfel_negligible_in_tile's verdict (s3 >= limit && s2 >= limit) is decided where each side that the verdict hangs on lies
# NEG_MARGIN x its conditioning clear of the limit, RELATIVE to the larger of the two. The device forms a side from the
# record's words in about ten rounded binary32 operations (aspect, dx0, U0, b, two fmas of P0, the constant C1, the fma of the
# centre value, the half-range, the subtraction; then a square, an fma and a product): each of lx, ly, hz, dx, dy carries at
# most 10 e of the summed magnitudes of its terms, a square doubles it, the quotient adds hz's share: (2 x 10 + 2 x 10 + 3) e
# = 2.6e-6 of a side whose terms do not cancel; v_rcp_f32 (1 ulp = 2 e) and, on the limit, v_log_f32 (1 ulp of a number of
# about 25: 1.2e-7 relative) and the conversion of cmax are inside the factor of four that 1e-5 leaves, as KEEP_MARGIN leaves
# one. Where the terms DO cancel (p's centre value is a difference of viewport-size coordinates; mean - b is one too) the
# error is relative to the terms, not to the result: negligible_terms reports that ratio (>= 1) per side and the margin is
# multiplied by it.
NEG_MARGIN = 1e-5
SURFEL_CULL_LOG2 = 23.0
STAGE_C1, STAGE_C2 = float(np.float32(0.84932180028801907)), float(np.float32(1.2011224087864498))   # stage_surfel's constants, as binary32 holds them


def keep_figure(case, rec, tx, ty):
    """raster_tile's separating-axis test in float64: the quad misses the box of the tile's sample positions where the larger of
    (|u_c| - e_u, |v_c| - e_v) exceeds 1.0001 (u, v in units of the quad's limit; tile centre, half extent 7.5 + the samples' reach).
    A NaN keeps the record (every compare is false)."""
    f = rec.astype(np.float64)
    half = 7.5 + {1: 0.0, 2: 0.25, 4: 0.375, 8: 0.4375}[case.samples]
    dcx, dcy = tx * TILE + 8.0 - f[0], ty * TILE + 8.0 - f[1]
    if case.variant == OBB:
        fu = abs(f[2] * dcx + f[3] * dcy) - half * (abs(f[2]) + abs(f[3]))
        fv = abs(f[4] * dcx + f[5] * dcy) - half * (abs(f[4]) + abs(f[5]))
    else:
        fu, fv = abs(f[2] * dcx) - half * abs(f[2]), abs(f[3] * dcy) - half * abs(f[3])
    return max(fu, fv) if np.isfinite(fu) and np.isfinite(fv) else -np.inf


def surfel_stage(case, rec, tx, ty):
    """stage_surfel in float64 from a record's raw words: the affine parts of p = P0 + Px xl + Py yl (p.xy scaled by C1) and of the
    screen-space deltas D = D0 + dD (xl, yl) (scaled by C2) over the tile's pixels xl, yl in [0, 15], with the magnitudes of
    what each P0 component and each D0 was summed from."""
    f = rec.astype(np.float64)
    cx, cy, m00, m11, radius, mx, my = f[0:7]
    Av, Bv, Cv = f[7:10], f[10:13], f[13:16]
    aspect = float(np.float32(case.viewport[0]) / np.float32(case.viewport[1]))
    U0, V0 = m00 * ((tx * TILE + 0.5) - cx), m11 * ((ty * TILE + 0.5) - cy)
    ax, bx = m00 * radius, U0 * radius + mx
    ay, by = m11 * radius * aspect, V0 * radius * aspect + my
    k = (STAGE_C1, STAGE_C1, 1.0)
    P0 = [k[i] * (Av[i] * bx + Bv[i] * by + Cv[i]) for i in range(3)]
    M0 = [k[i] * (abs(Av[i]) * (abs(U0 * radius) + abs(mx)) + abs(Bv[i]) * (abs(V0 * radius * aspect) + abs(my)) + abs(Cv[i])) for i in range(3)]
    Px = [k[i] * Av[i] * ax for i in range(3)]
    Py = [k[i] * Bv[i] * ay for i in range(3)]
    D0 = (STAGE_C2 * (mx - bx), STAGE_C2 * (my - by))
    MD = (STAGE_C2 * (2 * abs(mx) + abs(U0 * radius)), STAGE_C2 * (2 * abs(my) + abs(V0 * radius * aspect)))
    dD = (-STAGE_C2 * ax, -STAGE_C2 * ay)
    return {"P0": P0, "Px": Px, "Py": Py, "D0": D0, "dD": dD, "M0": M0, "MD": MD}


def negligible_terms(case, rec, tx, ty):
    """surfel_negligible_in_tile and frame_surfel_limit in float64, by the kernel's own interval construction: over the tile's
    pixel centres (centre H = 7.5, half-range H (|Px| + |Py|) of the affine part) |p.x|, |p.y| are at least lx, ly, |p.z| at most hz,
    the deltas at least dx, dy; s3 = (lx^2 + ly^2) / hz^2, s2 = dx^2 + dy^2 (exp2 units), limit = 23 + log2(max(1, cmax)).
    Returns (s3, s2, limit, cond3, cond2): cond is the ratio of a side's rounding error to its value in units of a side without
    cancellation (NEG_MARGIN). A NaN side stays NaN (the kernel keeps such a record)."""
    H = 7.5
    st = surfel_stage(case, rec, tx, ty)
    with np.errstate(all="ignore"):
        c = [st["P0"][i] + H * (st["Px"][i] + st["Py"][i]) for i in range(3)]
        e = [H * (abs(st["Px"][i]) + abs(st["Py"][i])) for i in range(3)]
        M = [st["M0"][i] + 2.0 * e[i] for i in range(3)]
        lx, ly, hz = max(abs(c[0]) - e[0], 0.0), max(abs(c[1]) - e[1], 0.0), abs(c[2]) + e[2]
        s3 = np.float64(lx * lx + ly * ly) / np.float64(hz * hz)
        num = lx * lx + ly * ly
        cond3 = max(1.0, (lx * M[0] + ly * M[1]) / num if num > 0.0 else 1.0, M[2] / hz if hz > 0.0 else 1.0)
        d, Md = [], []
        for j in range(2):
            d.append(max(abs(st["D0"][j] + H * st["dD"][j]) - H * abs(st["dD"][j]), 0.0))
            Md.append(st["MD"][j] + 2.0 * H * abs(st["dD"][j]))
        s2 = d[0] * d[0] + d[1] * d[1]
        cond2 = max(1.0, (d[0] * Md[0] + d[1] * Md[1]) / s2 if s2 > 0.0 else 1.0)
        cmax = float(np.uint32(case.color_max_bits).view(np.float32))
        limit = SURFEL_CULL_LOG2 + np.log2(cmax if cmax > 1.0 else 1.0)   # fmaxf(1, NaN) is 1
    return float(s3), float(s2), float(limit), float(cond3), float(cond2)


def negligible_figure(case, rec, tx, ty):
    """The smaller of (s3 - limit, s2 - limit) of negligible_terms: the record is dropped from the tile where this is >= 0 (not
    under the overlay, which drops nothing). -inf where a side is NaN: every compare is false and the record is kept."""
    s3, s2, limit, _, _ = negligible_terms(case, rec, tx, ty)
    return -np.inf if np.isnan(s3) or np.isnan(s2) else min(s3 - limit, s2 - limit)


def negligible_decided(case, rec, tx, ty):
    """Is the verdict NEG_MARGIN clear: a side clearly below the limit keeps the record whatever the other says; otherwise both
    must be clearly above."""
    s3, s2, limit, c3, c2 = negligible_terms(case, rec, tx, ty)
    if np.isnan(s3) or np.isnan(s2):
        return False
    below = lambda s, c: limit - s > NEG_MARGIN * c * max(s, limit)
    above = lambda s, c: s - limit > NEG_MARGIN * c * max(s, limit)
    return below(s3, c3) or below(s2, c2) or (above(s3, c3) and above(s2, c2))


def cost_reference(case, tx, ty, states):
    """What the regular wave of tile (tx, ty) must report, from the scan loop of raster_tile restated in integers:
        every group of 64 candidates that is queued costs WORK_GROUP; a group is queued when its hits fit the 64-entry queue;
        the queue is staged as one round when it holds FLUSH_AT = 32 or more, when the next group does not fit, or at the
        list's end: WORK_ROUND + WORK_STAGED per staged record + WORK_BLENDED per record that is kept (the quad reaches the
        tile's samples, a surfel drawn without the overlay is not negligible in the tile (negligible_figure < 0), and under a
        depth buffer z >= the tile's smallest depth); the tile stops after a round that leaves every pixel below the cut-off
        (bit 15) or when list and queue are empty.
    Returns {"work" (mode 0: without a mid-round exit), "saturated", "rounds", "countable"}; countable: every keep verdict lies
    KEEP_MARGIN clear of the slack, every surfel's negligible verdict NEG_MARGIN clear of the limit (negligible_decided) and
    every round-end saturation verdict is decided (`states`: render_reference's, for this case). The verdict and the rounds
    are the same in modes 1 and 2: a mid-round exit leaves only when every pixel is below the cut-off, which the round's end
    then finds too."""
    W = work_constants()
    s = (ty // case.sup_edge) * case.sup_x + tx // case.sup_edge
    total = min(int(case.totals[s]), case.cap)
    pos, ranks = case.tile_entries(tx, ty)
    st = states.get((tx, ty), [])
    dmin = None
    if case.depth is not None:
        dmin = case.depth[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].min()
    countable = True
    kept = []
    for rank in ranks:
        rec = case.records[int(rank)]
        fig = keep_figure(case, rec, tx, ty)
        countable &= abs(fig - KEEP_SLACK) > KEEP_MARGIN
        k = fig <= KEEP_SLACK
        if k and case.variant == SURFEL and not case.overlay:   # (a quad that misses the tile is not asked)
            countable &= negligible_decided(case, rec, tx, ty)
            k = negligible_figure(case, rec, tx, ty) < 0.0
        if dmin is not None:
            k = k and bool(np.float32(rec[20 if case.variant == SURFEL else 11]) >= dmin)
        kept.append(k)
    work = rounds = qn = base = done = 0
    saturated = False
    while True:
        have = base < total
        hits = int(((pos >= base) & (pos < base + 64)).sum()) if have else 0
        fits = qn + hits <= 64
        if have and fits:
            qn += hits
            work += W["group"]
            base += 64
        end = base >= total
        if qn and (qn >= 32 or not fits or end):
            work += W["round"] + qn * W["staged"] + W["blended"] * sum(kept[done:done + qn])
            done += qn
            qn = 0
            rounds += 1
            sat, decided = st[done - 1][:2]
            countable &= decided
            if sat:
                saturated = True
                break
        if end and qn == 0:
            break
    return {"work": min(work, 0x7FFF), "saturated": saturated, "rounds": rounds, "countable": bool(countable)}


def cost_references(case):
    """cost_reference of every tile of a case (row-major, as cost_out is indexed)."""
    states = {}
    render_reference(case, states=states)
    return [cost_reference(case, tx, ty, states) for ty in range(case.tiles_y) for tx in range(case.tiles_x)]


def _quad_matrix(case, rec):
    """(m00, m01, m10, m11) of the quad's uv = M (pixel - centre): the OBB record's, or the axis-aligned square's of a surfel."""
    f = rec.astype(np.float64)
    return (f[2], f[3], f[4], f[5]) if case.variant == OBB else (f[2], 0.0, 0.0, f[3])


def interior_figure(case, rec, tx, ty):
    """The largest |u| or |v| over the tile's pixel centres plus the samples' margin, in float64: a record is interior to the
    tile where this is <= 0.9999 (raster_tile; OBB: |u_c| + 7.5 (|m00| + |m01|) + margin, the surfel square: the corner values
    + 0.375 max(|du|, |dv|) at 4 samples)."""
    f = rec.astype(np.float64)
    m00, m01, m10, m11 = _quad_matrix(case, rec)
    ccx, ccy = tx * TILE + 8.0 - f[0], ty * TILE + 8.0 - f[1]
    offs = SAMPLE_OFFSETS[case.samples]
    if case.variant == OBB:
        mg = max(max(abs(m00 * ox + m01 * oy) for ox, oy in offs), max(abs(m10 * ox + m11 * oy) for ox, oy in offs))
    else:
        mg = {1: 0.0, 2: 0.25, 4: 0.375, 8: 0.4375}[case.samples] * max(abs(m00), abs(m11))
    fu = abs(m00 * ccx + m01 * ccy) + 7.5 * (abs(m00) + abs(m01)) + mg
    fv = abs(m10 * ccx + m11 * ccy) + 7.5 * (abs(m10) + abs(m11)) + mg
    return max(fu, fv)


def strip_reach(case, rec, tx, ty):
    """For each of the tile's four 16 x 4 strips: does any SAMPLE of the strip lie inside the OBB quad (float64, exact)."""
    f = rec.astype(np.float64)
    out = []
    for r in range(4):
        ys, xs = np.meshgrid(ty * TILE + 4 * r + np.arange(4) + 0.5, tx * TILE + np.arange(16) + 0.5, indexing="ij")
        any_ = False
        for ox, oy in SAMPLE_OFFSETS[case.samples]:
            dx, dy = xs + ox - f[0], ys + oy - f[1]
            m00, m01, m10, m11 = _quad_matrix(case, rec)
            any_ |= bool(((np.abs(m00 * dx + m01 * dy) <= 1.0) & (np.abs(m10 * dx + m11 * dy) <= 1.0)).any())
        out.append(any_)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def surfel_record(cx, cy, half, sx, sy, rgb=(1.0, 1.0, 1.0), a=0.5, z=0.5):
    """A RecordSurfel: the square quad of half extent `half` px around (cx, cy) and, in it, a surfel that faces the camera with
    standard deviations (sx, sy) px around the quad's centre: T0 = (sx, 0, cx), T1 = (0, sy, cy), T2 = (0, 0, 1), radius = half,
    mean = the centre; with a viewport aspect of 1 the pixel's own position is what meets the plane."""
    r = np.zeros(24, np.float32)
    r[0:4] = (cx, cy, 1.0 / half, 1.0 / half)
    r[4], r[5], r[6] = half, cx, cy
    T0, T1, T2 = np.array([sx, 0.0, cx]), np.array([0.0, sy, cy]), np.array([0.0, 0.0, 1.0])
    r[7:10], r[10:13], r[13:16] = np.cross(T1, T2), np.cross(T2, T0), np.cross(T0, T1)
    r[16:19], r[19], r[20] = rgb, a, z
    return r


def surfel_record_from_rows(cx, cy, half, T0, T1, T2, mean, rgb=(1.0, 1.0, 1.0), a=0.5, z=0.5):
    """A RecordSurfel from the three rows of a surfel's local-to-pixel matrix: the square quad of half extent `half` around
    (cx, cy), radius = half, the cross products A = T1 x T2, B = T2 x T0, C = T0 x T1 formed in float64 and rounded once."""
    r = np.zeros(24, np.float32)
    r[0:4] = (cx, cy, 1.0 / half, 1.0 / half)
    r[4], r[5], r[6] = half, mean[0], mean[1]
    T0, T1, T2 = (np.asarray(t, np.float64) for t in (T0, T1, T2))
    r[7:10], r[10:13], r[13:16] = np.cross(T1, T2), np.cross(T2, T0), np.cross(T0, T1)
    r[16:19], r[19], r[20] = rgb, a, z
    return r


def tilted_surfel_record(cx, cy, half, sx, sy, tilt, spin, mean_offset=(0.0, 0.0), focal=256.0, rgb=(1.0, 1.0, 1.0), a=0.5, z=0.5):
    """A RecordSurfel of a surfel that does NOT face the camera. The camera is a pinhole of `focal` pixels whose axis meets the
    image at pixel (0, 0): K = diag(focal, focal, 1). The surfel's centre lies at depth 1 on the ray of mean = (cx, cy) +
    mean_offset: c = (mean.x / focal, mean.y / focal, 1). Its first tangent is the in-plane direction e = (cos spin, sin spin, 0)
    tilted by `tilt` towards the viewing axis, d_u = cos tilt e + sin tilt z, its second the in-plane direction orthogonal to
    e, d_v = (-sin spin, cos spin, 0); a standard deviation of sx (sy) pixels at depth 1 is a length of sx / focal (sy / focal):
    t_u = sx d_u / focal, t_v = sy d_v / focal. A point (s, t) of the surfel, in standard deviations, is c + s t_u + t t_v, and
    its homogeneous pixel is K [t_u t_v c] (s, t, 1): the rows of that matrix are
        T0 = (sx d_u.x, sy d_v.x, mean.x),  T1 = (sx d_u.y, sy d_v.y, mean.y),  T2 = (sx d_u.z / focal, 0, 1),
    written so that focal is divided by only where it does not cancel. The pixel pc sees the surfel at (s, t) = p.xy / p.z
    with p = (pc.x T2 - T0) x (pc.y T2 - T1) = pc.x A + pc.y B + C. With a tilt p.z = C.z + A.z pc.x + B.z pc.y varies over the
    image, A.z = -sx sy sin tilt cos spin / focal and B.z = -sx sy sin tilt sin spin / focal, and vanishes on the surfel
    plane's horizon, the line pc . (cos spin, sin spin) = focal / tan tilt: the default focal keeps it about 100 px from the
    origin at a tilt of 1.2. The quad stays the square around (cx, cy) and pc = pixel + mean_offset, so the screen-space side
    is 2 |pixel - (cx, cy)|^2 whatever the offset. tilt = 0 and no offset give surfel_record's words bit for bit."""
    ct, st_, cs, ss = np.cos(tilt), np.sin(tilt), np.cos(spin), np.sin(spin)
    mean = (cx + mean_offset[0], cy + mean_offset[1])
    du = (ct * cs, ct * ss, st_)
    dv = (0.0 - ss, cs)   # (0 - sin: no negative zero at spin 0)
    T0 = (sx * du[0], sy * dv[0], mean[0])
    T1 = (sx * du[1], sy * dv[1], mean[1])
    T2 = (sx * du[2] / focal, 0.0, 1.0)
    return surfel_record_from_rows(cx, cy, half, T0, T1, T2, mean, rgb, a, z)


def surfel_sides(case, rec, tx, ty):
    """(p [3 grids], s3, s2) of a surfel record over the pixel centres of tile (tx, ty) in float64, by _record_terms' own
    expressions: s3 = |p.xy / p.z|^2 (inf or NaN where p.z == 0), s2 = 2 |mean - pc|^2."""
    f = rec.astype(np.float64)
    ys, xs = np.meshgrid(ty * TILE + np.arange(TILE) + 0.5, tx * TILE + np.arange(TILE) + 0.5, indexing="ij")
    aspect = float(np.float32(case.viewport[0]) / np.float32(case.viewport[1]))
    ex, ey = f[2] * (xs - f[0]) * f[4], f[3] * (ys - f[1]) * f[4] * aspect
    pcx, pcy = ex + f[5], ey + f[6]
    p = [f[7 + i] * pcx + f[10 + i] * pcy + f[13 + i] for i in range(3)]
    with np.errstate(all="ignore"):
        s3 = (p[0] / p[2]) ** 2 + (p[1] / p[2]) ** 2
    return p, s3, 2.0 * (ex * ex + ey * ey)


def _fma32(a, b, c):
    """fmaf of binary32 operands: the product is exact in float64, the sum rounds to float64 and then to binary32 (one rounding
    wherever the sum fits 53 bits, which is every use here: operands of a few bits each)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def stage_surfel32(case, rec, tx, ty):
    """stage_surfel operation by operation in binary32 (the kernel's own order, fmaf where it has one): the staged words
    P0 [3], Px [3], Py [3], with `inner` = the three sums before the constant C1 multiplies them."""
    f = rec.astype(np.float32)
    one = np.float32
    ox, oy = one(tx * TILE + 0.5), one(ty * TILE + 0.5)
    aspect = one(case.viewport[0]) / one(case.viewport[1])
    U0, V0 = f[2] * (ox - f[0]), f[3] * (oy - f[1])
    radius = f[4]
    ax, bx = f[2] * radius, _fma32(U0, radius, f[5])
    ay, by = f[2 + 1] * radius * aspect, _fma32(V0 * radius, aspect, f[6])
    A, B, C = f[7:10], f[10:13], f[13:16]
    C1 = one(STAGE_C1)
    inner = [_fma32(A[i], bx, _fma32(B[i], by, C[i])) for i in range(3)]
    P0 = [C1 * inner[0], C1 * inner[1], inner[2]]
    Px = [C1 * A[0] * ax, C1 * A[1] * ax, A[2] * ax]
    Py = [C1 * B[0] * ay, C1 * B[1] * ay, B[2] * ay]
    return {"U0": U0, "V0": V0, "ax": ax, "bx": bx, "ay": ay, "by": by, "inner": inner, "P0": P0, "Px": Px, "Py": Py}


def pixel_p32(st, qx, qy):
    """p at pixel (qx, qy) of the tile from stage_surfel32's words, as blend_px forms it: fma(Py, qy, fma(Px, qx, P0))."""
    return [_fma32(st["Py"][i], np.float32(qy), _fma32(st["Px"][i], np.float32(qx), st["P0"][i])) for i in range(3)]


SPINS = (0.5, 2.2, -1.1, 3.9)   # one per quadrant: (A.z, B.z) take every pair of signs, |cos|, |sin| >= 0.45


def _tilt_interior_records():
    """Four quads that hold tile (0, 0) of a 32 x 32 target with room to spare, their surfels tilted by 0.6 and 1.2, spun into
    the four quadrants, means a few pixels off the quad centres."""
    spec = ((9.1, 7.3, 40, 14, 11, 0.6, (3.0, -2.0)), (8.3, 8.9, 50, 17, 12, 1.2, (-2.5, 1.5)),
            (7.2, 8.4, 45, 12, 15, 1.2, (1.5, 3.0)), (8.8, 6.9, 42, 16, 10, 0.6, (-3.0, -1.0)))
    return np.array([tilted_surfel_record(cx, cy, half, sx, sy, tilt, SPINS[i], off, rgb=PRIMARIES[i], a=0.4)
                     for i, (cx, cy, half, sx, sy, tilt, off) in enumerate(spec)], np.float32)


def surfel_tilted_cases():
    """The designed surfel cases again with planes that do not face the camera (tilted_surfel_record): p.z varies from pixel
    to pixel, A.z and B.z differ in sign and size, the mean is off the quad centre, the viewport's aspect is not 1."""
    out = []
    full = rect(0, 1, 0, 1)
    # a. interior quads: the hand-written interior update at 1 and 4 samples, blend_px / blend_px_ms in the sort rasteriser and at 2, 8
    recs = _tilt_interior_records()
    for S in (1, 2, 4, 8):
        lists, totals = make_lists([[(i, full) for i in range(4)]])
        out.append(Case(f"surfel_tilt_interior_s{S}", 32, 32, recs, lists, totals, samples=S, variant=SURFEL,
                        notes={"interior": {(0, 0): [True] * 4}, "tilted": [0, 1, 2, 3]}))
    for S in (1, 4):
        # b. surfel_cover_strips' and surfel_cover_room_to_spare's quads (the strips first: test_strip_cases reads record 4 as
        # the quad smaller than a pixel). The small quads carry surfels larger than themselves behind a short focal length, so
        # that A.z, B.z stay well above rounding; tilt 0.6 keeps their horizon 90 px away.
        small = lambda i, cx, cy, half: tilted_surfel_record(cx, cy, half, 3.0, 2.5, 0.6, SPINS[i % 4], (0.4, -0.3), focal=64.0, rgb=PRIMARIES[i], a=0.5)
        recs = np.array([small(0, 8.2, 1.3, 1.1), small(1, 7.7, 14.6, 1.0), small(2, 8.1, 8.0, 0.7), small(3, 16.0, 16.0, 0.3),
                         small(4, 5.5 + 0.01, 9.5 - 0.02, 0.25),
                         tilted_surfel_record(9.1, 7.3, 40, 14, 11, 1.2, SPINS[1], (2.0, 1.0), rgb=PRIMARIES[5], a=0.3),
                         tilted_surfel_record(5.3, 5.1, 4.3, 4.5, 3.6, 0.6, SPINS[2], (-0.5, 0.7), focal=64.0, rgb=PRIMARIES[1], a=0.5),
                         tilted_surfel_record(8.3, 8.9, 50, 17, 12, 0.6, SPINS[3], (-2.0, 2.5), rgb=PRIMARIES[2], a=0.3)], np.float32)
        lists, totals = make_lists([[(i, full) for i in range(8)]])
        out.append(Case(f"surfel_tilt_edge_and_strips_s{S}", 32, 32, recs, lists, totals, samples=S, variant=SURFEL,
                        notes={"interior": {(0, 0): [False] * 5 + [True, False, True]}, "tilted": list(range(8)),
                               "strips": {0: [True, False, False, False], 1: [False, False, False, True], 2: [False, True, True, False]},
                               "misses_tile": {3: [(0, 0), (1, 0), (0, 1), (1, 1)] if S == 1 else [(1, 0), (0, 1)]}}))
        # c. case a's records under viewports of aspect 1.5 and 2 / 3, neither of the target's size
        for name, vp in (("3_2", (48.0, 32.0)), ("2_3", (32.0, 48.0))):
            lists, totals = make_lists([[(i, full) for i in range(4)]])
            out.append(Case(f"surfel_tilt_aspect_{name}_s{S}", 32, 32, _tilt_interior_records(), lists, totals, samples=S, variant=SURFEL, viewport=vp,
                            notes={"interior": {(0, 0): [True] * 4}, "tilted": [0, 1, 2, 3]}))
        # d. one standard deviation of 0.5 px (under 1 / sqrt 2: along it the screen-space side 2 d^2 is the smaller) and one of
        # 12 px (along it the surfel's own side is): min(s3, s2) takes either on a good part of tile (0, 0)
        recs = np.array([tilted_surfel_record(8.3, 7.6, 40, 12.0, 0.5, 1.2, 0.6, (0.3, -0.2), rgb=PRIMARIES[3], a=0.6),
                         tilted_surfel_record(7.4, 8.7, 44, 0.55, 9.0, 0.6, 2.5, (-0.4, 0.25), rgb=PRIMARIES[4], a=0.6)], np.float32)
        lists, totals = make_lists([[(i, full) for i in range(2)]])
        out.append(Case(f"surfel_tilt_filter_crossover_s{S}", 32, 32, recs, lists, totals, samples=S, variant=SURFEL,
                        notes={"interior": {(0, 0): [True, True]}, "tilted": [0, 1], "crossover_tile": (0, 0)}))
        # e. surfel_cover_alternating_kinds_* with tilted planes: runs of interior and of other records, p.z varying in both
        for first in (True, False):
            recs, kinds = [], []
            for i in range(64):
                interior = (i % 2 == 0) == first
                kinds.append(interior)
                if interior:
                    recs.append(tilted_surfel_record(8.1 + 0.01 * i, 7.9, 60, 20 + 0.1 * i, 25 - 0.1 * i, 0.6 if i % 4 < 2 else 1.2, SPINS[(i // 2) % 4],
                                                     (2.0 - 0.05 * i, -1.5 + 0.04 * i), rgb=PRIMARIES[i % 6], a=0.08))
                else:
                    recs.append(tilted_surfel_record(2.0 + (i % 7) * 2.0 + 0.1, 3.0 + (i % 5) * 2.5 + 0.05, 3.1, 3.3, 2.7, 0.6, SPINS[(i // 2) % 4],
                                                     (0.3, -0.4), focal=64.0, rgb=PRIMARIES[i % 6], a=0.5))
            lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(64)]])
            out.append(Case(f"surfel_tilt_alternating_kinds_{'interior' if first else 'other'}_first_s{S}", 16, 16, np.array(recs, np.float32), lists, totals,
                            samples=S, variant=SURFEL, notes={"interior": {(0, 0): kinds}, "tilted": list(range(64))}))
    return out


def surfel_negligible_cases():
    """What surfel_negligible_in_tile takes out of a tile: two thin ellipses (20 x 0.6 px standard deviations) in 64 x 64 quads
    on 4 x 4 tiles, one facing the camera along x, one tilted by 1.2 and a little turned. The tiles along an ellipse blend it,
    the tiles a few standard deviations to its side do not (rows 0 and 3; in row 2 the two tiles next to the quad centre keep it,
    the screen-space side being below the limit there);`notes["blended"]` says which, per tile and record. The quad centres are placed so
    that the outer tiles of row 2 lie between the limits of cmax = 1 (23) and cmax = 6 (25.58): tiles (0, 2) and (3, 2) drop
    record 0 and tile (0, 2) record 1 at cmax 1 and blend them at cmax 6 (`notes["flips"]`). Under the overlay nothing is
    dropped."""
    recs = np.array([tilted_surfel_record(32.3, 29.05, 32, 20.0, 0.6, 0.0, 0.0, (0.5, -0.25), focal=512.0, rgb=PRIMARIES[0], a=0.6),
                     tilted_surfel_record(32.3, 28.75, 32, 20.0, 0.6, 1.2, 0.15, (0.5, -0.25), focal=512.0, rgb=PRIMARIES[2], a=0.6)], np.float32)
    rows_1 = {0: [(False, False)] * 4, 1: [(True, True)] * 4, 2: [(False, False), (True, True), (True, True), (False, False)], 3: [(False, False)] * 4}
    rows_6 = dict(rows_1)
    rows_6[2] = [(True, True), (True, True), (True, True), (True, False)]
    blended = lambda rows: {(tx, ty): list(rows[ty][tx]) for ty in range(4) for tx in range(4)}
    out = []
    for name, S, cmax, overlay, rows in (("cmax_1_s1", 1, 1.0, 0, rows_1), ("cmax_1_s4", 4, 1.0, 0, rows_1), ("cmax_6_s1", 1, 6.0, 0, rows_6),
                                         ("overlay_s1", 1, 1.0, 1, None)):
        lists, totals = make_lists([[(i, rect(0, 3, 0, 3)) for i in range(2)]])
        notes = {"tilted": [1], "blended": blended(rows) if rows else {(tx, ty): [True, True] for ty in range(4) for tx in range(4)}}
        if name == "cmax_6_s1":
            notes["flips"] = [(0, 0, 2), (0, 3, 2), (1, 0, 2)]   # (record, tx, ty) dropped at cmax 1, blended here
        out.append(Case(f"surfel_negligible_{name}", 64, 64, recs, lists, totals, samples=S, variant=SURFEL, overlay=overlay,
                        color_max_bits=float_bits(cmax), notes=notes))
    return out


def surfel_grazing_cases():
    """Rays that graze a surfel's plane inside the tile: p.z passes through 0, v_rcp_f32 returns huge values, inf and (times a
    zero) NaN, and min(s3, s2) must come out as the screen-space side. 16 x 16, one tile, 1 and 4 samples. Not designed cases:
    next to the horizon the reference's bound grows as the kernel's error does, and a pixel whose bound exceeds 2^-10 (the
    whole-frame render tolerance) is left out of the float64 comparison — `notes["horizon"]`; never out of the bit comparison.
      i.  two surfels tilted by 1.45 whose horizons cross the tile obliquely between pixel centres, one in a quad that holds
          the tile (the interior update), one in a 12 px quad (blend_px).
      ii. power-of-two words, every staged operation on the way to p.z exact. Record 0, rows T0 = (2, 0, 7), T1 = (0, 2, 8),
          T2 = (1/4, 0, 1) in a quad around (8.5, 8.5): pc = the pixel's index - (1, 0), p.z = 4 - pc.x / 2 = 0 on column 9 while
          p.x = 2 pc.x - 14 = 2 there: an inf quotient, s3 = inf; named pixel (9, 8), one pixel from the quad centre. p is the
          cofactor matrix of [T0 T1 T2] applied to (pc, 1), so p.xyz = 0 needs a singular matrix: record 1 has T0 = (1, 0, 4) =
          4 T2, the surfel's plane through the eye, p = (pc.x - 4) (2, 2, -1/2) with pc.x = column: 0 x inf = NaN on column 4;
          named pixel (4, 8), the quad centre (4.5, 8.5). One record cannot hold both: where the matrix is singular p.z = 0
          only where all of p is. The constant C1 scales p.xy by a binary32 number: a zero stays a zero and a power of two times
          it is exact, so record 1's p.x, p.y are exact zeros on the device as well."""
    out = []
    for S in (1, 4):
        recs = np.array([tilted_surfel_record(8.3, 7.6, 40, 6.0, 5.0, 1.45, 0.3, (0.3, -0.2), focal=78.0, rgb=PRIMARIES[0], a=0.5),
                         tilted_surfel_record(7.2, 8.4, 6.0, 5.0, 4.0, 1.45, -0.4, (-0.25, 0.3), focal=62.4, rgb=PRIMARIES[2], a=0.5)], np.float32)
        lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(2)]])
        out.append(Case(f"surfel_grazing_oblique_s{S}", 16, 16, recs, lists, totals, samples=S, variant=SURFEL, notes={"interior": {(0, 0): [True, False]}}))
        recs = np.array([surfel_record_from_rows(8.5, 8.5, 16.0, (2.0, 0.0, 7.0), (0.0, 2.0, 8.0), (0.25, 0.0, 1.0), (7.0, 8.0), PRIMARIES[3], 0.5),
                         surfel_record_from_rows(4.5, 8.5, 16.0, (1.0, 0.0, 4.0), (0.0, 2.0, 8.0), (0.25, 0.0, 1.0), (4.0, 8.0), PRIMARIES[4], 0.5)], np.float32)
        out.append(Case(f"surfel_grazing_exact_s{S}", 16, 16, recs, lists.copy(), totals.copy(), samples=S, variant=SURFEL,
                        notes={"interior": {(0, 0): [True, True]}, "inf_pixel": (0, 9, 8), "nan_pixel": (1, 4, 8)}))   # (record, x, y)
    return out


def surfel_coverage_cases():
    """Interior / edge / strips for the surfel variant, 1 and 4 samples: the cases of coverage_cases() with square quads (a
    surfel's quad is axis-aligned, so there is no turned quad; the thin quad is a small square across the strips' boundary).
    viewport 32 x 32: aspect 1."""
    out = []
    for S in (1, 4):
        m = 0.375 if S == 4 else 0.0
        recs = np.array([surfel_record(9.1, 7.3, 40, 14, 11, PRIMARIES[0], 0.5), surfel_record(5.3, 5.1, 4.3, 1.5, 1.2, PRIMARIES[1], 0.5),
                         surfel_record(8.3, 8.9, 50, 17, 12, PRIMARIES[2], 0.5)], np.float32)
        lists, totals = make_lists([[(i, rect(0, 1, 0, 1)) for i in range(3)]])
        out.append(Case(f"surfel_cover_room_to_spare_s{S}", 32, 32, recs, lists, totals, samples=S, variant=SURFEL,
                        notes={"interior": {(0, 0): [True, False, True]}}))
        inside, outside = (7.5 + m) / 0.9998, (7.5 + m) / 1.00005
        recs = np.array([surfel_record(8.0, 8.0, inside, 4.0, 3.0, PRIMARIES[3], 0.5), surfel_record(8.0, 8.0, outside, 3.0, 4.0, PRIMARIES[4], 0.5)], np.float32)
        lists, totals = make_lists([[(0, rect(0, 1, 0, 1)), (1, rect(0, 1, 0, 1))]])
        out.append(Case(f"surfel_cover_threshold_straddle_s{S}", 32, 32, recs, lists, totals, samples=S, variant=SURFEL,
                        notes={"interior": {(0, 0): [True, False]}}))
        for first in (True, False):
            recs, kinds = [], []
            for i in range(64):
                interior = (i % 2 == 0) == first
                kinds.append(interior)
                if interior:
                    recs.append(surfel_record(8.1 + 0.01 * i, 7.9, 60, 20 + 0.1 * i, 25 - 0.1 * i, PRIMARIES[i % 6], 0.08))
                else:
                    recs.append(surfel_record(2.0 + (i % 7) * 2.0 + 0.1, 3.0 + (i % 5) * 2.5 + 0.05, 3.1, 1.1, 0.9, PRIMARIES[i % 6], 0.5))
            lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(64)]])
            out.append(Case(f"surfel_cover_alternating_kinds_{'interior' if first else 'other'}_first_s{S}", 16, 16, np.array(recs, np.float32), lists, totals,
                            samples=S, variant=SURFEL, notes={"interior": {(0, 0): kinds}}))
        recs = np.array([surfel_record(8.2, 1.3, 1.1, 0.5, 0.4, PRIMARIES[0], 0.5), surfel_record(7.7, 14.6, 1.0, 0.4, 0.5, PRIMARIES[1], 0.5),
                         surfel_record(8.1, 8.0, 0.7, 0.3, 0.3, PRIMARIES[2], 0.5), surfel_record(16.0, 16.0, 0.3, 0.2, 0.2, PRIMARIES[3], 0.5),
                         surfel_record(5.5 + 0.01, 9.5 - 0.02, 0.25, 0.1, 0.1, PRIMARIES[4], 0.5)], np.float32)
        lists, totals = make_lists([[(i, rect(0, 1, 0, 1)) for i in range(5)]])
        out.append(Case(f"surfel_cover_strips_s{S}", 32, 32, recs, lists, totals, samples=S, variant=SURFEL,
                        notes={"strips": {0: [True, False, False, False], 1: [False, False, False, True], 2: [False, True, True, False]},
                               "misses_tile": {3: [(0, 0), (1, 0), (0, 1), (1, 1)] if S == 1 else [(1, 0), (0, 1)]}}))
    return out


def _grid_records(n, tx=0, ty=0, a=0.5, variant=OBB, size=2.0):
    """n small quads cycling over the 16 cells (4 x 4 px) of tile (tx, ty), adjacent records in distinct primaries: no pixel is
    covered by more than ceil(n / 16) of them, so nothing saturates below 13 x 16 records, and any reordering, drop or
    duplicate moves a pixel by about alpha / 2."""
    recs = []
    for i in range(n):
        cell = i % 16
        cx = tx * TILE + (cell % 4) * 4 + 2.0 + 0.25 * ((i // 16) % 3)   # (centres off the pixel and sample grids)
        cy = ty * TILE + (cell // 4) * 4 + 2.0 + 0.0625 + 0.25 * ((i // 48) % 3)
        rgb = PRIMARIES[i % 6]
        if variant == OBB:
            recs.append(obb_record(cx + 0.03, cy + 0.02, size + 0.013, size + 0.017, 0.1 * (i % 5), rgb, a))
        else:
            recs.append(aabb_record(cx + 0.03, cy + 0.02, 1.0 / (size + 0.013), 1.0 / (size + 0.017), 1.0, 0.2, 1.5, rgb, a))
    return np.array(recs, np.float32).reshape(-1, 12)


def list_total_cases():
    out = []
    for total in (0, 1, 63, 64, 65, 127, 128, 129, 192, 193):
        recs = _grid_records(max(total, 1))
        lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(total)]], cap=max(total, 1))
        out.append(Case(f"list_total_{total}", 16, 16, recs, lists, totals, notes={"group_hits": [min(64, total - g) for g in range(0, total, 64)]}))
    return out


def list_edge_cases():
    out = []
    # a total above the cap: list 0 says 70 with a cap of 64; what lies behind the cap is list 1, bright records whose
    # rectangles name tile 0 and whose own total is 0
    recs = np.concatenate([_grid_records(64), np.array([obb_record(8, 8, 30, 30, 0, BRIGHT, 0.9)] * 6, np.float32)])
    lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(64)], [(64 + i, rect(0, 1, 0, 0)) for i in range(6)]], cap=64)
    totals[:] = (70, 0)
    out.append(Case("list_total_above_cap", 32, 16, recs, lists, totals, sup_edge=1, notes={"never_drawn": list(range(64, 70))}))
    # RECT_EMPTY entries in the middle of a list: bright ranks that touch no tile
    recs = np.concatenate([_grid_records(40), np.array([obb_record(8, 8, 30, 30, 0, BRIGHT, 0.9)], np.float32)])
    entries = []
    for i in range(40):
        entries.append((i, rect(0, 0, 0, 0)))
        if i % 7 == 3:
            entries.append((40, np.uint32(RECT_EMPTY)))
    lists, totals = make_lists([entries])
    out.append(Case("list_rect_empty_inside", 16, 16, recs, lists, totals, notes={"never_drawn": [40]}))
    # inclusive limits on 3 x 3 tiles: every record covers the whole target, its rectangle says where it is drawn
    big = lambda i, a: obb_record(24.3, 24.1, 200, 200, 0.3, PRIMARIES[i], a)
    rects = [rect(1, 1, 1, 1), rect(0, 1, 0, 2), rect(1, 2, 0, 2), rect(0, 2, 0, 1), rect(0, 2, 1, 2), rect(2, 2, 0, 0)]
    recs = np.array([big(i, 0.3 + 0.1 * i) for i in range(6)], np.float32)
    lists, totals = make_lists([[(i, rects[i]) for i in range(6)]])
    out.append(Case("list_rect_limits_inclusive", 48, 48, recs, lists, totals, notes={"per_tile": {(1, 1): [0, 1, 2, 3, 4], (0, 0): [1, 3], (2, 0): [2, 3, 5],
                                                                                                     (0, 2): [1, 4], (2, 2): [2, 4]}}))
    # supertile edges 1 and 2 on 4 x 3 tiles: every list holds its own record (covering everything, rectangle everything)
    for edge in (1, 2):
        sx, sy = -(-4 // edge), -(-3 // edge)
        n = sx * sy
        recs = np.array([obb_record(32.2, 24.4, 300, 300, 0.2, (0.1 + 0.07 * s, 1.0 - 0.06 * s, 0.03 * s * s % 1.0), 0.6) for s in range(n)], np.float32)
        lists, totals = make_lists([[(s, rect(0, 3, 0, 2))] for s in range(n)])
        out.append(Case(f"list_sup_edge_{edge}", 64, 48, recs, lists, totals, sup_edge=edge, notes={"own_list_only": True}))
    # 17 supertiles in a row
    recs = np.array([obb_record(136.1, 8.2, 900, 900, 0.1, (0.05 * s, 1.0 - 0.05 * s, (0.31 * s) % 1.0), 0.7) for s in range(17)], np.float32)
    lists, totals = make_lists([[(s, rect(0, 16, 0, 0))] for s in range(17)])
    out.append(Case("list_17_supertiles_in_a_row", 272, 16, recs, lists, totals, sup_edge=1, notes={"own_list_only": True}))
    return out


def queue_cases():
    """Hits per 64-candidate group of tile 0's list; the misses name tile 1 (of a 32 x 16 target) and are drawn there."""
    out = []
    for name, pattern in (("31", [31]), ("32", [32]), ("33", [33]), ("64", [64]), ("40_40", [40, 40]), ("1_x_40", [1] * 40), ("0_64", [0, 64])):
        entries, recs, k = [], [], 0
        hits = _grid_records(sum(pattern), 0, 0)
        for g, nh in enumerate(pattern):
            last = g == len(pattern) - 1
            slots = nh if last and nh else 64
            where = set(np.linspace(0, slots - 1, nh).astype(int).tolist()) if nh else set()
            for i in range(slots):
                if i in where:
                    recs.append(hits[k]); k += 1
                    entries.append((len(recs) - 1, rect(0, 0, 0, 0)))
                else:
                    j = len(recs)
                    recs.append(_grid_records(j + 1, 1, 0)[j])
                    entries.append((j, rect(1, 1, 0, 0)))
        assert k == sum(pattern)
        lists, totals = make_lists([entries])
        out.append(Case(f"queue_hits_{name}", 32, 16, np.array(recs, np.float32), lists, totals, modes=(0, 2), notes={"group_hits": pattern}))
    return out


def coverage_cases():
    """Interior / edge / strips, OBB, 1 and 4 samples (2 x 2 tiles; the tile looked at is (0, 0) unless said)."""
    out = []
    for S in (1, 4):
        mg = {1: 0.0, 4: 0.5}[S]   # |du| of a sample, in px, for an axis-aligned quad: at most 0.375 (a turned one: 0.5)
        # a record that covers the tile with room to spare, behind and in front of edge records
        recs = np.array([obb_record(9.1, 7.3, 40, 40, 0.4, PRIMARIES[0], 0.5), obb_record(5.2, 5.1, 4.3, 3.1, 0.7, PRIMARIES[1], 0.5),
                         obb_record(8.3, 8.9, 35, 50, 1.1, PRIMARIES[2], 0.5)], np.float32)
        lists, totals = make_lists([[(i, rect(0, 1, 0, 1)) for i in range(3)]])
        out.append(Case(f"cover_room_to_spare_s{S}", 32, 32, recs, lists, totals, samples=S, modes=(0, 1, 2) if S in (1, 4) else (0,),
                        notes={"interior": {(0, 0): [True, False, True]}}))
        # two axis-aligned records that straddle the 0.9999 threshold at tile (0, 0): centre on the tile centre, the figure is
        # (7.5 + margin) / half: just inside with half = (7.5 + m) / 0.9998, just outside with half = (7.5 + m) / 1.00005
        m = 0.375 if S == 4 else 0.0
        inside, outside = (7.5 + m) / 0.9998, (7.5 + m) / 1.00005
        recs = np.array([obb_record(8.0, 8.0, inside, inside, 0.0, PRIMARIES[3], 0.5), obb_record(8.0, 8.0, outside, outside, 0.0, PRIMARIES[4], 0.5)], np.float32)
        lists, totals = make_lists([[(0, rect(0, 1, 0, 1)), (1, rect(0, 1, 0, 1))]])
        out.append(Case(f"cover_threshold_straddle_s{S}", 32, 32, recs, lists, totals, samples=S, notes={"interior": {(0, 0): [True, False]}}))
        # interior, other, interior ... over all 64 slots of a round; then the same with the kinds swapped (records 0 and 63 of either kind)
        for first in (True, False):
            recs, kinds = [], []
            for i in range(64):
                interior = (i % 2 == 0) == first
                kinds.append(interior)
                if interior:
                    recs.append(obb_record(8.1 + 0.01 * i, 7.9, 60, 60, 0.05 * i, PRIMARIES[i % 6], 0.08))
                else:
                    recs.append(obb_record(2.0 + (i % 7) * 2.0 + 0.1, 3.0 + (i % 5) * 2.5 + 0.05, 3.1, 2.2, 0.3 * i, PRIMARIES[i % 6], 0.5))
            lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(64)]])
            out.append(Case(f"cover_alternating_kinds_{'interior' if first else 'other'}_first_s{S}", 16, 16, np.array(recs, np.float32), lists, totals,
                            samples=S, modes=(0, 1, 2), notes={"interior": {(0, 0): kinds}}))
        # strips: only strip 0, only strip 3, a thin quad along the boundary between strips 1 and 2, a 45-degree quad whose
        # rectangle holds a corner tile it misses, a quad smaller than a pixel (on a pixel centre)
        recs = np.array([obb_record(8.2, 1.3, 6.0, 1.1, 0.0, PRIMARIES[0], 0.5), obb_record(7.7, 14.6, 5.0, 1.0, 0.0, PRIMARIES[1], 0.5),
                         obb_record(8.1, 8.0, 7.0, 0.7, 0.0, PRIMARIES[2], 0.5), obb_record(16.0, 16.0, 14.0, 0.3, np.pi / 4, PRIMARIES[3], 0.5),
                         obb_record(5.5 + 0.01, 9.5 - 0.02, 0.3, 0.2, 0.2, PRIMARIES[4], 0.5)], np.float32)
        lists, totals = make_lists([[(i, rect(0, 1, 0, 1)) for i in range(5)]])
        out.append(Case(f"cover_strips_s{S}", 32, 32, recs, lists, totals, samples=S, modes=(0, 2),
                        notes={"strips": {0: [True, False, False, False], 1: [False, False, False, True], 2: [False, True, True, False]},
                               "misses_tile": {3: [(1, 0), (0, 1)]}}))
    return out


def exact_edge_cases():
    """AABB3D with power-of-two coefficients: |u| == 1 exactly on a pixel centre (1 sample) and on a sample (4 samples)."""
    out = []
    # centre (8, 8), m = 1/4: u = (x + 0.5 - 8) / 4 = +-1 at x + 0.5 = 12, 4 — pixel centres are at .5: use centre 8.5: |u| = 1 at 4.5 and 12.5
    recs = np.array([aabb_record(8.5, 8.5, 0.25, 0.25, 1.0, 0.0, 1.0, PRIMARIES[0], 0.5)], np.float32)
    lists, totals = make_lists([[(0, rect(0, 0, 0, 0))]])
    out.append(Case("exact_edge_on_pixel_centre_s1", 16, 16, recs, lists, totals, variant=AABB3D, modes=(0, 1), notes={"edge_pixels": [(4, 8), (12, 8), (8, 4), (8, 12)]}))
    # 4 samples: sample 1 is at (+0.375, -0.125) of the centre; centre 8.5 + 0.375 - 4 ... : cx = 8.875 puts sample 1 of pixel x = 12 at u = (12.5 + 0.375 - 8.875) / 4 = 1
    recs = np.array([aabb_record(8.875, 8.375, 0.25, 0.25, 1.0, 0.0, 1.0, PRIMARIES[1], 0.5)], np.float32)
    out.append(Case("exact_edge_on_sample_s4", 16, 16, recs, lists.copy(), totals.copy(), variant=AABB3D, samples=4, modes=(0, 1), notes={"edge_pixels": [(12, 8)]}))
    return out


def _opaque(cx, cy, hx, hy, rgb):
    return obb_record(cx, cy, hx, hy, 0.0, rgb, 1.0)   # alpha clamps to 0.999 wherever exp(-4.5 q) >= 0.999: q <= 2.2e-4


def saturation_cases():
    """Records that clamp alpha to 0.999 over the whole tile (half extents of 4000 px: q < 2e-5) take T through 1, 1e-3, 1e-6."""
    out = []
    wide = lambda rgb: _opaque(8.0, 8.0, 4000.0, 4000.0, rgb)
    small = lambda i: obb_record(2.0 + (i % 6) * 2.3, 2.5 + (i % 5) * 2.7, 0.9, 0.8, 0.1 * i, PRIMARIES[i % 6], 0.25)
    for at in (2, 4, 5, 64, 70):   # the tile saturates after this many records of its list (70: in the second round)
        recs = [small(i) for i in range(at - 2)] + [wide((0.5, 0.25, 0.125)), wide((0.25, 0.5, 0.75))] + [wide(BRIGHT) for _ in range(6)]
        lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(len(recs))]])
        out.append(Case(f"saturate_after_{at}", 16, 16, np.array(recs, np.float32), lists, totals, modes=(0, 1, 2), color_max_bits=float_bits(4.0),
                        notes={"saturates_after": at - 1, "never_adds": list(range(at, at + 6))}))
    recs = [small(0), wide((0.5, 0.25, 0.125)), wide((0.25, 0.5, 0.75))] + [wide((64.0, 64.0, 64.0))] * 3
    lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(len(recs))]])
    out.append(Case("saturate_cmax_64", 16, 16, np.array(recs, np.float32), lists, totals, modes=(0, 1, 2), color_max_bits=float_bits(64.0),
                    notes={"saturates_after": 2, "t_eps": 2.0 ** -17, "never_adds": [3, 4, 5]}))
    # a round that ends with every pixel a little ABOVE the cut-off (T = 1e-3 x 0.3 = 2.5 t_eps, less under the small quads): the
    # tile must go on, and the second round's record shows at about 1e-4, thousands of times the bound. A cut-off taken a few
    # times too high leaves here.
    recs = [small(i) for i in range(62)] + [wide((0.5, 0.25, 0.125)), obb_record(8.0, 8.0, 4000.0, 4000.0, 0.0, (0.25, 0.5, 0.75), 0.7)] + \
           [obb_record(8.0, 8.0, 4000.0, 4000.0, 0.0, PRIMARIES[3], 0.4)]
    lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(len(recs))]])
    out.append(Case("saturate_not_yet_at_2p5_t_eps", 16, 16, np.array(recs, np.float32), lists, totals, modes=(0, 1, 2),
                    notes={"saturates_after": None, "above_cutoff_after": 63}))
    # only the left half of the tile saturates: the records behind still draw on the right half
    half = lambda rgb: obb_record(-4000.0 + 7.75, 8.0, 4000.0, 4000.0, 0.0, rgb, 1.0)   # right edge at x = 7.75: between pixel centres
    recs = [half((0.5, 0.25, 0.125)), half((0.25, 0.5, 0.75))] + [obb_record(8.0, 8.0, 4000.0, 4000.0, 0.0, PRIMARIES[i % 6] * 4.0, 0.4) for i in range(5)]
    lists, totals = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(len(recs))]])
    out.append(Case("saturate_half_tile", 16, 16, np.array(recs, np.float32), lists, totals, modes=(0, 1, 2), color_max_bits=float_bits(4.0),
                    notes={"saturates_after": None}))
    return out


def strip_workgroup_cases():
    """Tiles that need more than one staging round (> 64 kept records, none saturating), drawn by their regular waves and, in
    modes 1 and 2, by strip workgroups — and with a reversed workgroup order. 1 and 4 samples; one under a depth buffer."""
    out = []
    rng = np.random.default_rng(11)
    for S, with_depth in ((1, False), (4, False), (4, True), (1, True)):
        recs = np.concatenate([_grid_records(150, 1, 0, a=0.4), _grid_records(20, 0, 1, a=0.4)])
        recs[:, 11] = np.linspace(0.9, 0.1, len(recs)).astype(np.float32)
        entries = [(i, rect(1, 1, 0, 0)) for i in range(150)] + [(150 + i, rect(0, 0, 1, 1)) for i in range(20)]
        lists, totals = make_lists([entries])
        depth = None
        if with_depth:
            depth = rng.uniform(0.3, 0.7, (32, 48, S)).astype(np.float32)
        out.append(Case(f"strips_heavy_tile_s{S}{'_depth' if with_depth else ''}", 48, 32, recs, lists, totals, samples=S, modes=(1, 2), depth=depth,
                        heavy_tiles=(1,), notes={"rounds": {(1, 0): 3}}))
    return out


def depth_cases():
    out = []
    for S in (1, 2, 4, 8):
        rng = np.random.default_rng(100 + S)
        depth = rng.uniform(0.4, 0.6, (16, 32, S)).astype(np.float32)
        depth[:, 16:, :] = np.float32(0.5)   # tile 1: one depth everywhere
        zs = [0.7, 0.3, 0.5, float(depth[5, 6, 0]), 0.45, 0.55]   # above dmax, below dmin, between, equal to one sample's depth
        recs = np.array([obb_record(10.2 + 2 * i, 8.1, 9.0, 7.0, 0.3 * i, PRIMARIES[i], 0.5, z) for i, z in enumerate(zs)], np.float32)
        lists, totals = make_lists([[(i, rect(0, 1, 0, 0)) for i in range(len(zs))]])
        out.append(Case(f"depth_s{S}", 32, 16, recs, lists, totals, samples=S, depth=depth, modes=(0, 1, 2) if S in (1, 4) else (0,),
                        notes={"z": zs}))
    return out


def shape_cases():
    out = []
    for w, h in ((1, 1), (17, 15), (40, 24)):
        tx, ty = -(-w // 16), -(-h // 16)
        recs = np.array([obb_record(w * 0.4 + 0.3, h * 0.6 + 0.2, w * 0.7 + 1, h * 0.5 + 1, 0.5, PRIMARIES[0], 0.5),
                         obb_record(w * 0.7, h * 0.2, 3.3, 2.2, 1.0, PRIMARIES[1], 0.6),
                         obb_record(w - 0.6, h - 0.4, 2.5, 2.5, 0.0, PRIMARIES[2], 0.7)], np.float32)
        lists, totals = make_lists([[(i, rect(0, tx - 1, 0, ty - 1)) for i in range(3)]])
        for S in (1, 4):
            out.append(Case(f"shape_{w}x{h}_s{S}", w, h, recs, lists.copy(), totals.copy(), samples=S, modes=(0, 2)))
    return out


def honest_rect(case_w, case_h, cx, cy, ex, ey):
    """The packed rectangle of the tiles the box centre +- extent touches, or RECT_EMPTY."""
    tx, ty = -(-case_w // 16), -(-case_h // 16)
    x0, x1 = int(np.floor((cx - ex) / 16)), int(np.floor((cx + ex) / 16))
    y0, y1 = int(np.floor((cy - ey) / 16)), int(np.floor((cy + ey) / 16))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, tx - 1), min(y1, ty - 1)
    return np.uint32(RECT_EMPTY) if x0 > x1 or y0 > y1 else rect(x0, x1, y0, y1)


def mixed_records(variant, n=200, seed=5, w=64, h=48):
    """About 200 random records of a variant on a w x h target with honest rectangles, front to back."""
    rng = np.random.default_rng(seed)
    recs, rects = [], []
    for i in range(n):
        cx, cy = rng.uniform(-4, w + 4), rng.uniform(-4, h + 4)
        hx, hy = np.exp(rng.uniform(np.log(0.6), np.log(30.0), 2))
        rgb = rng.uniform(0.0, 1.0, 3)
        a = rng.uniform(0.05, 1.0)
        z = rng.uniform(0.05, 0.95)
        if variant == OBB:
            th = rng.uniform(0, np.pi)
            recs.append(obb_record(cx, cy, hx, hy, th, rgb, a, z))
            ext = abs(np.cos(th)) * hx + abs(np.sin(th)) * hy, abs(np.sin(th)) * hx + abs(np.cos(th)) * hy
        elif variant == AABB3D:
            A, C = rng.uniform(2.0, 9.0, 2)
            B = rng.uniform(-0.9, 0.9) * np.sqrt(A * C)
            recs.append(aabb_record(cx, cy, 1.0 / hx, 1.0 / hy, A, B, C, rgb, a, z))
            ext = hx, hy
        else:   # a surfel record: quad as AABB3D; a plane facing the camera through the quad centre, in the record's own terms
            hh = max(hx, hy)
            r = np.zeros(24, np.float32)
            r[0:4] = (cx, cy, 1.0 / hh, 1.0 / hh)
            r[4], r[5], r[6] = hh, cx, cy                      # radius, mean
            # T0 = (sx, 0, mean.x), T1 = (0, sy, mean.y), T2 = (0, 0, 1): A = T1 x T2, B = T2 x T0, C = T0 x T1
            sx, sy = hx / 3.0, hy / 3.0
            T0, T1, T2 = np.array([sx, 0.0, cx]), np.array([0.0, sy, cy]), np.array([0.0, 0.0, 1.0])
            r[7:10], r[10:13], r[13:16] = np.cross(T1, T2), np.cross(T2, T0), np.cross(T0, T1)
            r[16:19], r[19], r[20] = rgb, a, z
            recs.append(r)
            ext = hh, hh
        rects.append(honest_rect(w, h, cx, cy, ext[0] + 1.0, ext[1] + 1.0))
    return np.array(recs, np.float32), np.array(rects, np.uint32)


def instantiations():
    """(variant, samples, depth, overlay, mode) of every untraced instantiation of raster_scan_kernel that RasterInst::exists
    (csrc/frame_params.h) admits: the exit instantiations exist for OBB (1, 2) and AABB3D (1) at 1 or 4 samples without overlay."""
    out = []
    for variant in (OBB, AABB3D, SURFEL):
        for S in (1, 2, 4, 8):
            for depth in (False, True):
                for overlay in (0, 1):
                    modes = (0,)
                    if variant != SURFEL and S in (1, 4) and not overlay:
                        modes = (0, 1, 2) if variant == OBB else (0, 1)
                    for mode in modes:
                        out.append((variant, S, depth, overlay, mode))
    return out


def mixed_case(variant, S, depth, overlay, mode, seed=5):
    w, h = 64, 48
    recs, rects = mixed_records(variant, seed=seed, w=w, h=h)
    per = [[] for _ in range(4)]
    for i, rc in enumerate(rects):   # sup_edge 2 on 4 x 3 tiles: 2 x 2 supertiles; a rank goes to the lists its rectangle overlaps
        if rc == RECT_EMPTY:
            continue
        x0, x1, y0, y1 = int(rc) & 255, (int(rc) >> 8) & 255, (int(rc) >> 16) & 255, int(rc) >> 24
        for sy in range(y0 // 2, y1 // 2 + 1):
            for sx in range(x0 // 2, x1 // 2 + 1):
                per[sy * 2 + sx].append((i, rc))
    lists, totals = make_lists(per)
    d = None
    if depth:
        d = np.random.default_rng(seed + 77).uniform(0.2, 0.8, (h, w, S)).astype(np.float32)
    return Case(f"mixed_v{variant}_s{S}{'_depth' if depth else ''}{'_overlay' if overlay else ''}_m{mode}", w, h, recs, lists, totals, sup_edge=2,
                samples=S, variant=variant, overlay=overlay, modes=(mode,), depth=d, random=True)


def mixed_tilted_records(n=200, seed=5, w=64, h=48):
    """mixed_records' surfels again, none of them facing the camera by design: tilts uniform in [0, 1.3], any spin, the mean up
    to 2 px off the quad centre, behind a focal length of 512 px (the horizon of a tilt of 1.3 is 142 px from the origin; the
    target's far corner, offsets included, is 86)."""
    rng = np.random.default_rng(seed)
    recs, rects = [], []
    for i in range(n):
        cx, cy = rng.uniform(-4, w + 4), rng.uniform(-4, h + 4)
        hx, hy = np.exp(rng.uniform(np.log(0.6), np.log(30.0), 2))
        rgb = rng.uniform(0.0, 1.0, 3)
        a = rng.uniform(0.05, 1.0)
        z = rng.uniform(0.05, 0.95)
        tilt, spin = rng.uniform(0.0, 1.3), rng.uniform(0.0, 2.0 * np.pi)
        off = rng.uniform(-2.0, 2.0, 2)
        hh = max(hx, hy)
        recs.append(tilted_surfel_record(cx, cy, hh, hx / 3.0, hy / 3.0, tilt, spin, (off[0], off[1]), focal=512.0, rgb=rgb, a=a, z=z))
        rects.append(honest_rect(w, h, cx, cy, hh + 1.0, hh + 1.0))
    return np.array(recs, np.float32), np.array(rects, np.uint32)


def tilted_instantiations():
    """(samples, depth, overlay) of every surfel instantiation."""
    return [(S, depth, overlay) for S in (1, 2, 4, 8) for depth in (False, True) for overlay in (0, 1)]


def mixed_tilted_case(S, depth, overlay, seed=5):
    w, h = 64, 48
    recs, rects = mixed_tilted_records(seed=seed, w=w, h=h)
    per = [[] for _ in range(4)]
    for i, rc in enumerate(rects):   # as mixed_case: 2 x 2 supertiles of 2 x 2 tiles
        if rc == RECT_EMPTY:
            continue
        x0, x1, y0, y1 = int(rc) & 255, (int(rc) >> 8) & 255, (int(rc) >> 16) & 255, int(rc) >> 24
        for sy in range(y0 // 2, y1 // 2 + 1):
            for sx in range(x0 // 2, x1 // 2 + 1):
                per[sy * 2 + sx].append((i, rc))
    lists, totals = make_lists(per)
    d = None
    if depth:
        d = np.random.default_rng(seed + 77).uniform(0.2, 0.8, (h, w, S)).astype(np.float32)
    return Case(f"mixed_tilted_s{S}{'_depth' if depth else ''}{'_overlay' if overlay else ''}", w, h, recs, lists, totals, sup_edge=2,
                samples=S, variant=SURFEL, overlay=overlay, depth=d, random=True)


def nan_case():
    """A record whose cx is NaN in the middle of a list, and the same list without it."""
    recs = _grid_records(30)
    nan = obb_record(np.nan, 8.0, 5.0, 5.0, 0.2, BRIGHT, 0.9)
    with_nan = np.concatenate([recs[:15], nan[None], recs[15:]])
    a, ta = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(31)]])
    b, tb = make_lists([[(i, rect(0, 0, 0, 0)) for i in range(30)]])
    return (Case("nan_cx_inside_list", 16, 16, with_nan, a, ta, modes=(0, 2)), Case("nan_cx_twin_without", 16, 16, recs, b, tb, modes=(0, 2)))


def designed_cases():
    return (list_total_cases() + list_edge_cases() + queue_cases() + coverage_cases() + exact_edge_cases() + saturation_cases() +
            strip_workgroup_cases() + depth_cases() + shape_cases() + surfel_coverage_cases() + surfel_tilted_cases() + surfel_negligible_cases())
