"""Independent numpy/Python model of the line-segment detection stage (the checker of tests/test_lsd_host.py and
tests/test_gpu_lsd.py), written from the contract in DESIGN §11 rather than from the GPU code:

  gray_rgb          CV_RGB2GRAY on 8U: (R*4899 + G*9617 + B*1868 + 8192) >> 14, first channel = R
  resize_u8         INTER_LINEAR on 8U, the fixed-point form (11-bit coefficients, rounding shift by 22)
  gauss_kernel      getGaussianKernel(7, sigma_scale / scale) in double: 0.6 / 0.8 = 0.7499999999999999, not 0.75
  blur              separable 7-tap fp64 filter, BORDER_REFLECT_101: rows with the taps summed left to right, then
                    columns in the symmetric form (centre tap, then k[j] * (S[+j] + S[-j]))
  resize_f64        INTER_LINEAR by 0.8 on doubles (float coefficients), rows then columns
  fast_atan2        the float polynomial in degrees
  ll_angle          gradient, norm, angle, NOTDEF; last row and column NOTDEF
  lsd               the LSD_REFINE_ADV walk: seeds in raster order, region_grow with the running angle, region2rect,
                    refine / reduce_region_radius, rect_improve, rect_nfa; +0.5, /0.8, float
  detect            items 1-4 of the contract: grey, max-width downscale, LSD, upscale, length filter, priority-queue
                    order, cap
  stages            every stage of one image on its own: grey, small, blur, float degrees, modgrad, the raw list, and the
                    counts of the walk (seeds, nfa_evals, max_grad, which branches were taken)

Pure Python region growing: small images only (a 480x360 frame takes seconds).
"""
import math

import numpy as np

NOTDEF = -1024.0
DEG_TO_RADS = math.pi / 180
SCALE = 0.8
SIGMA_SCALE = 0.6
QUANT = 2.0
ANG_TH = 22.5
LOG_EPS = 0.0
DENSITY_TH = 0.7
F32 = np.float32
DBL_EPS_F = F32(np.finfo(np.float64).eps)
_R2D = F32(180.0 / math.pi)
P1 = F32(0.9997878412794807) * _R2D
P3 = F32(-0.3258083974640975) * _R2D
P5 = F32(0.1555786518463281) * _R2D
P7 = F32(-0.04432655554792128) * _R2D


# ---- fastAtan2: float32 arithmetic, every operation rounded -------------------------------------------------------
def fast_atan2(y, x):
    """scalar or array; float32 in, float32 degrees in [0, 360) out"""
    y = np.asarray(y, F32)
    x = np.asarray(x, F32)
    ax, ay = np.abs(x), np.abs(y)
    def poly(c):
        cc = c * c
        return (((P7 * cc + P5) * cc + P3) * cc + P1) * c
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = np.where(ax >= ay, poly(ay / (ax + DBL_EPS_F)), F32(90.0) - poly(ax / (ay + DBL_EPS_F))).astype(F32)
    a = np.where(x < 0, F32(180.0) - a, a).astype(F32)
    a = np.where(y < 0, F32(360.0) - a, a).astype(F32)
    return a


# ---- grey and the 8U downscale ------------------------------------------------------------------------------------
def gray_rgb(img):
    img = np.asarray(img)
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def _round_half_even(v):
    return int(np.rint(v))


def resize_size(n, f):
    """dsize of cv::resize(src, dst, Size(), f, f) along one axis"""
    return _round_half_even(n * f)


def resize_map(n_dst, n_src, inv_scale):
    """INTER_LINEAR source index and float weight per destination index (fx = float((d+0.5)*scale - 0.5))"""
    scale = 1.0 / inv_scale
    sx = np.zeros(n_dst, np.int64)
    fx = np.zeros(n_dst, F32)
    for d in range(n_dst):
        f = F32((d + 0.5) * scale - 0.5)
        s = math.floor(f)
        f = F32(f - F32(s))
        if s < 0:
            s, f = 0, F32(0)
        if s >= n_src - 1:
            s, f = n_src - 1, F32(0)
        sx[d], fx[d] = s, f
    return sx, fx


def _coef_u8(f):
    return np.rint(np.asarray(f, F32) * F32(2048)).astype(np.int64)


def resize_u8(g, new_w, new_h, inv_scale):
    h, w = g.shape
    sx, fx = resize_map(new_w, w, inv_scale)
    sy, fy = resize_map(new_h, h, inv_scale)
    a0, a1 = _coef_u8(F32(1) - fx), _coef_u8(fx)
    b0, b1 = _coef_u8(F32(1) - fy), _coef_u8(fy)
    gi = g.astype(np.int64)
    sx1 = np.minimum(sx + 1, w - 1)
    hor = gi[:, sx] * a0 + gi[:, sx1] * a1                      # [h, new_w]
    sy1 = np.minimum(sy + 1, h - 1)
    v = (hor[sy] * b0[:, None] + hor[sy1] * b1[:, None] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


def downscale(g, max_image_width):
    """-> (image handed to LSD, upscale_x, upscale_y) as Line3D::detectLineSegments computes them"""
    rows, cols = g.shape
    max_dim = max(rows, cols)
    if max_image_width > 0 and max_dim > max_image_width:
        s = F32(max_image_width) / F32(max_dim)
        nw, nh = resize_size(cols, float(s)), resize_size(rows, float(s))
        r = resize_u8(g, nw, nh, float(s))
        return r, F32(cols) / F32(nw), F32(rows) / F32(nh)
    return g, F32(1), F32(1)


# ---- blur and the 0.8 resample ------------------------------------------------------------------------------------
def gauss_kernel(n=7, sigma=SIGMA_SCALE / SCALE):
    """lsd_opencv.cpp:550 divides in double: sigma is one ulp under 0.75, and three of the four distinct taps differ from
    those of 0.75 in the last place"""
    scale2x = -0.5 / (sigma * sigma)
    xs = [i - (n - 1) * 0.5 for i in range(n)]
    t = [math.exp(scale2x * x * x) for x in xs]
    s = 0.0
    for v in t:
        s += v
    s = 1.0 / s
    return np.array([v * s for v in t])


def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def blur(img):
    k = gauss_kernel()
    img = img.astype(np.float64)
    h, w = img.shape
    cx = [np.array([reflect101(x + t - 3, w) for x in range(w)]) for t in range(7)]
    acc = k[0] * img[:, cx[0]]
    for t in range(1, 7):
        acc = acc + k[t] * img[:, cx[t]]
    # columns: OpenCV's symmetric column filter, centre tap first, then k[3+j] * (S[y+j] + S[y-j]) for j = 1, 2, 3
    out = k[3] * acc
    for j in range(1, 4):
        up = np.array([reflect101(y + j, h) for y in range(h)])
        dn = np.array([reflect101(y - j, h) for y in range(h)])
        out = out + k[3 + j] * (acc[up] + acc[dn])
    return out


def resize_f64(b, scale=SCALE):
    h, w = b.shape
    nw, nh = resize_size(w, scale), resize_size(h, scale)
    sx, fx = resize_map(nw, w, scale)
    sy, fy = resize_map(nh, h, scale)
    a0, a1 = (F32(1) - fx).astype(np.float64), fx.astype(np.float64)
    b0, b1 = (F32(1) - fy).astype(np.float64), fy.astype(np.float64)
    hor = b[:, sx] * a0 + b[:, np.minimum(sx + 1, w - 1)] * a1
    return hor[sy] * b0[:, None] + hor[np.minimum(sy + 1, h - 1)] * b1[:, None]


def ll_angle(s):
    """-> (angles in radians as double with NOTDEF, degrees float32 with NOTDEF, modgrad, max_grad)"""
    h, w = s.shape
    rho = QUANT / math.sin(math.pi * ANG_TH / 180)
    DA = s[1:, 1:] - s[:-1, :-1]
    BC = s[:-1, 1:] - s[1:, :-1]
    gx = DA + BC
    gy = DA - BC
    norm = np.sqrt((gx * gx + gy * gy) / 4)
    deg = np.full((h, w), F32(NOTDEF), F32)
    mod = np.zeros((h, w))
    mod[:-1, :-1] = norm
    a = fast_atan2(gx.astype(F32), (-gy).astype(F32))
    defined = norm > rho
    deg[:-1, :-1] = np.where(defined, a, F32(NOTDEF))
    ang = np.where(deg == F32(NOTDEF), NOTDEF, deg.astype(np.float64) * DEG_TO_RADS)
    max_grad = float(norm[defined].max()) if defined.any() else -1.0
    return ang, deg, mod, max_grad


# ---- the walk -----------------------------------------------------------------------------------------------------
def _log_gamma(x):
    if x > 15.0:
        return 0.918938533204673 + (x - 0.5) * math.log(x) - x + 0.5 * x * math.log(x * math.sinh(1 / x) + 1 / (810.0 * math.pow(x, 6.0)))
    q = (75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424, 2.50662827511)
    a = (x + 0.5) * math.log(x + 5.5) - (x + 5.5)
    b = 0.0
    for n in range(7):
        a -= math.log(x + float(n))
        b += q[n] * math.pow(x, float(n))
    return a + math.log(b)


def _double_equal(a, b):
    if a == b:
        return True
    d = abs(a - b)
    m = max(abs(a), abs(b))
    if m < 2.2250738585072014e-308:
        m = 2.2250738585072014e-308
    return d / m <= 100.0 * 2.220446049250313e-16


def _angle_diff_signed(a, b):
    d = a - b
    while d <= -math.pi:
        d += 2 * math.pi
    while d > math.pi:
        d -= 2 * math.pi
    return d


def _tdiv(a, b):
    """C integer division (truncation toward zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


class _Rect:
    __slots__ = ("x1", "y1", "x2", "y2", "width", "x", "y", "theta", "dx", "dy", "prec", "p")

    def copy(self):
        r = _Rect()
        for k in self.__slots__:
            setattr(r, k, getattr(self, k))
        return r


class LSD:
    def __init__(self, scaled):
        self.h, self.w = scaled.shape
        self.ang, self.deg, self.mod, self.max_grad = ll_angle(scaled)
        self.angf = self.ang.reshape(-1).tolist()
        self.modf = self.mod.reshape(-1).tolist()
        self.used = bytearray(self.w * self.h)
        self.LOG_NT = 5 * (math.log10(float(self.w)) + math.log10(float(self.h))) / 2 + math.log10(11.0)
        self.nfa_evals = 0
        self.seeds = 0                     # regions grown from a seed in run (not the re-grow inside refine)
        # branches taken, for the tests that need to know a scene reaches them: refine's re-grow, reduce_region_radius,
        # a refine that fails, and rect_improve's exits (after 1 evaluation, then after each later stage)
        self.regrown = self.reduced = self.refine_failed = 0
        self.improve_exits = [0] * 6

    def aligned(self, adr, theta, prec):
        a = self.angf[adr]
        if a == NOTDEF:
            return False
        t = theta - a
        if t < 0:
            t = -t
        if t > 3 * math.pi / 2:
            t -= 2 * math.pi
            if t < 0:
                t = -t
        return t <= prec

    def region_grow(self, sx, sy, prec):
        W, H = self.w, self.h
        adr = sx + sy * W
        reg = [(sx, sy)]
        ang = self.angf[adr]
        reg_angle = ang
        sumdx = F32(math.cos(reg_angle))
        sumdy = F32(math.sin(reg_angle))
        self.used[adr] = 1
        i = 0
        while i < len(reg):
            px, py = reg[i]
            for yy in range(max(py - 1, 0), min(py + 1, H - 1) + 1):
                for xx in range(max(px - 1, 0), min(px + 1, W - 1) + 1):
                    c = xx + yy * W
                    if self.used[c] != 1 and self.aligned(c, reg_angle, prec):
                        self.used[c] = 1
                        reg.append((xx, yy))
                        a = float(F32(self.angf[c]))
                        sumdx = F32(float(sumdx) + math.cos(a))
                        sumdy = F32(float(sumdy) + math.sin(a))
                        reg_angle = float(fast_atan2(sumdy, sumdx)) * DEG_TO_RADS
            i += 1
        return reg, reg_angle

    def get_theta(self, reg, x, y, reg_angle, prec):
        Ixx = Iyy = Ixy = 0.0
        W = self.w
        for (px, py) in reg:
            wgt = self.modf[px + py * W]
            dx = float(px) - x
            dy = float(py) - y
            Ixx += dy * dy * wgt
            Iyy += dx * dx * wgt
            Ixy -= dx * dy * wgt
        assert not (_double_equal(Ixx, 0) and _double_equal(Iyy, 0) and _double_equal(Ixy, 0))
        lam = 0.5 * (Ixx + Iyy - math.sqrt((Ixx - Iyy) * (Ixx - Iyy) + 4.0 * Ixy * Ixy))
        if abs(Ixx) > abs(Iyy):
            th = float(fast_atan2(F32(lam - Ixx), F32(Ixy)))
        else:
            th = float(fast_atan2(F32(Ixy), F32(lam - Iyy)))
        th *= DEG_TO_RADS
        if abs(_angle_diff_signed(th, reg_angle)) > prec:
            th += math.pi
        return th

    def region2rect(self, reg, reg_angle, prec, p):
        W = self.w
        x = y = s = 0.0
        for (px, py) in reg:
            wgt = self.modf[px + py * W]
            x += float(px) * wgt
            y += float(py) * wgt
            s += wgt
        assert s > 0
        x /= s
        y /= s
        th = self.get_theta(reg, x, y, reg_angle, prec)
        dx, dy = math.cos(th), math.sin(th)
        lmin = lmax = wmin = wmax = 0.0
        for (px, py) in reg:
            rx, ry = float(px) - x, float(py) - y
            l = rx * dx + ry * dy
            w = -rx * dy + ry * dx
            if l > lmax:
                lmax = l
            elif l < lmin:
                lmin = l
            if w > wmax:
                wmax = w
            elif w < wmin:
                wmin = w
        r = _Rect()
        r.x1, r.y1 = x + lmin * dx, y + lmin * dy
        r.x2, r.y2 = x + lmax * dx, y + lmax * dy
        r.width = wmax - wmin
        r.x, r.y, r.theta, r.dx, r.dy, r.prec, r.p = x, y, th, dx, dy, prec, p
        if r.width < 1.0:
            r.width = 1.0
        return r

    @staticmethod
    def _dist(x1, y1, x2, y2):
        return math.sqrt((x2 - x1) * (x2 - x1) + (y2 - y1) * (y2 - y1))

    def refine(self, reg, reg_angle, prec, p, rec):
        W = self.w
        density = float(len(reg)) / (self._dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width)
        if density >= DENSITY_TH:
            return True, reg, rec
        xc, yc = float(reg[0][0]), float(reg[0][1])
        ang_c = self.angf[reg[0][0] + reg[0][1] * W]
        s = ss = 0.0
        n = 0
        for (px, py) in reg:
            self.used[px + py * W] = 0
            if self._dist(xc, yc, float(px), float(py)) < rec.width:
                d = _angle_diff_signed(self.angf[px + py * W], ang_c)
                s += d
                ss += d * d
                n += 1
        mean = s / float(n)
        tau = 2.0 * math.sqrt((ss - 2.0 * mean * s) / float(n) + mean * mean)
        self.regrown += 1
        reg, reg_angle = self.region_grow(reg[0][0], reg[0][1], tau)
        if len(reg) < 2:
            self.refine_failed += 1
            return False, reg, rec
        rec = self.region2rect(reg, reg_angle, prec, p)
        density = float(len(reg)) / (self._dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width)
        if density < DENSITY_TH:
            return self.reduce_region_radius(reg, reg_angle, prec, p, rec, density)
        return True, reg, rec

    def reduce_region_radius(self, reg, reg_angle, prec, p, rec, density):
        W = self.w
        self.reduced += 1
        reg = list(reg)
        xc, yc = float(reg[0][0]), float(reg[0][1])
        r1 = (rec.x1 - xc) * (rec.x1 - xc) + (rec.y1 - yc) * (rec.y1 - yc)
        r2 = (rec.x2 - xc) * (rec.x2 - xc) + (rec.y2 - yc) * (rec.y2 - yc)
        rad = r1 if r1 > r2 else r2
        n = len(reg)
        while density < DENSITY_TH:
            rad *= 0.75 * 0.75
            i = 0
            while i < n:
                px, py = reg[i]
                if (float(px) - xc) * (float(px) - xc) + (float(py) - yc) * (float(py) - yc) > rad:
                    self.used[px + py * W] = 0
                    reg[i], reg[n - 1] = reg[n - 1], reg[i]
                    n -= 1
                    i -= 1
                i += 1
            if n < 2:
                self.refine_failed += 1
                return False, reg[:n], rec
            rec = self.region2rect(reg[:n], reg_angle, prec, p)
            density = float(n) / (self._dist(rec.x1, rec.y1, rec.x2, rec.y2) * rec.width)
        return True, reg[:n], rec

    def nfa(self, n, k, p):
        LOG_NT = self.LOG_NT
        if n == 0 or k == 0:
            return -LOG_NT
        if n == k:
            return -LOG_NT - float(n) * math.log10(p)
        p_term = p / (1 - p)
        log1 = (float(n) + 1) - _log_gamma(float(k) + 1) - _log_gamma(float(n - k) + 1) \
            + float(k) * math.log(p) + float(n - k) * math.log(1.0 - p)
        term = math.exp(log1)
        if _double_equal(term, 0):
            return (-log1 / 2.30258509299404568402 - LOG_NT) if k > n * p else -LOG_NT
        tail = term
        for i in range(k + 1, n + 1):
            bt = float(n - i + 1) / float(i)
            mt = bt * p_term
            term *= mt
            tail += term
            if bt < 1:
                err = term * ((1 - math.pow(mt, float(n - i + 1))) / (1 - mt) - 1)
                if err < 0.1 * abs(-math.log10(tail) - LOG_NT) * tail:
                    break
        return -math.log10(tail) - LOG_NT

    def rect_nfa(self, rec):
        self.nfa_evals += 1
        hw = rec.width / 2.0
        dyhw, dxhw = rec.dy * hw, rec.dx * hw
        pts = [[int(rec.x1 - dyhw), int(rec.y1 + dxhw)], [int(rec.x2 - dyhw), int(rec.y2 + dxhw)],
               [int(rec.x2 + dyhw), int(rec.y2 - dxhw)], [int(rec.x1 + dyhw), int(rec.y1 - dxhw)]]
        pts.sort(key=lambda q: (q[0], q[1]))
        taken = [False] * 4
        mn = mx = 0
        for i in range(1, 4):
            if pts[mn][1] > pts[i][1]:
                mn = i
            if pts[mx][1] < pts[i][1]:
                mx = i
        taken[mn] = True

        def pick(better):
            sel = None
            for i in range(4):
                if not taken[i] and (sel is None or better(pts[sel][0], pts[i][0])):
                    sel = i
            taken[sel] = True
            return sel
        lm = pick(lambda cur, new: cur > new)
        rm = pick(lambda cur, new: cur < new)
        tl = pick(lambda cur, new: cur > new)
        MN, LM, RM, TL = pts[mn], pts[lm], pts[rm], pts[tl]
        flstep = float(_tdiv(MN[0] - LM[0], MN[1] - LM[1])) if MN[1] != LM[1] else 0.0
        slstep = float(_tdiv(LM[0] - TL[0], LM[1] - TL[0])) if LM[1] != TL[0] else 0.0
        frstep = float(_tdiv(MN[0] - RM[0], MN[1] - RM[1])) if MN[1] != RM[1] else 0.0
        srstep = float(_tdiv(RM[0] - TL[0], RM[1] - TL[0])) if RM[1] != TL[0] else 0.0
        lstep, rstep = flstep, frstep
        lx = rx = float(MN[0])
        total = alg = 0
        W, H = self.w, self.h
        th, pr = rec.theta, rec.prec
        for y in range(MN[1], pts[mx][1] + 1):
            if 0 <= y < H:
                x0, x1 = max(int(lx), 0), min(int(rx), W - 1)
                if x1 >= x0:
                    total += x1 - x0 + 1
                    base = y * W
                    for x in range(x0, x1 + 1):
                        if self.aligned(base + x, th, pr):
                            alg += 1
            if y >= LM[1]:
                lstep = slstep
            if y >= RM[1]:
                rstep = srstep
            lx += lstep
            rx += rstep
        return self.nfa(total, alg, rec.p)

    def rect_improve(self, rec):
        delta, d2 = 0.5, 0.25
        log_nfa = self.rect_nfa(rec)
        if log_nfa > LOG_EPS:
            self.improve_exits[0] += 1
            return log_nfa, rec
        r = rec.copy()
        for _ in range(5):
            r.p /= 2
            r.prec = r.p * math.pi
            v = self.rect_nfa(r)
            if v > log_nfa:
                log_nfa, rec = v, r.copy()
        if log_nfa > LOG_EPS:
            self.improve_exits[1] += 1
            return log_nfa, rec
        r = rec.copy()
        for _ in range(5):
            if r.width - delta >= 0.5:
                r.width -= delta
                v = self.rect_nfa(r)
                if v > log_nfa:
                    rec, log_nfa = r.copy(), v
        if log_nfa > LOG_EPS:
            self.improve_exits[2] += 1
            return log_nfa, rec
        for sign in (1.0, -1.0):
            r = rec.copy()
            for _ in range(5):
                if r.width - delta >= 0.5:
                    if sign > 0:
                        r.x1 += -r.dy * d2
                        r.y1 += r.dx * d2
                        r.x2 += -r.dy * d2
                        r.y2 += r.dx * d2
                    else:
                        r.x1 -= -r.dy * d2
                        r.y1 -= r.dx * d2
                        r.x2 -= -r.dy * d2
                        r.y2 -= r.dx * d2
                    r.width -= delta
                    v = self.rect_nfa(r)
                    if v > log_nfa:
                        rec, log_nfa = r.copy(), v
            if log_nfa > LOG_EPS:
                self.improve_exits[3 if sign > 0 else 4] += 1
                return log_nfa, rec
        r = rec.copy()
        for _ in range(5):
            if r.width - delta >= 0.5:
                r.p /= 2
                r.prec = r.p * math.pi
                v = self.rect_nfa(r)
                if v > log_nfa:
                    rec, log_nfa = r.copy(), v
        self.improve_exits[5] += 1
        return log_nfa, rec

    def run(self):
        prec = math.pi * ANG_TH / 180
        p = ANG_TH / 180
        min_reg = int(-self.LOG_NT / math.log10(p))
        W = self.w
        out = []
        for adr in range(W * self.h):          # raster order: flsd walks list[] by index
            if self.used[adr] != 0 or self.angf[adr] == NOTDEF:
                continue
            self.seeds += 1
            reg, reg_angle = self.region_grow(adr % W, adr // W, prec)
            if len(reg) < min_reg:
                continue
            rec = self.region2rect(reg, reg_angle, prec, p)
            ok, reg, rec = self.refine(reg, reg_angle, prec, p, rec)
            if not ok:
                continue
            log_nfa, rec = self.rect_improve(rec)
            if log_nfa <= LOG_EPS:
                continue
            out.append([F32((rec.x1 + 0.5) / SCALE), F32((rec.y1 + 0.5) / SCALE),
                        F32((rec.x2 + 0.5) / SCALE), F32((rec.y2 + 0.5) / SCALE)])
        return np.array(out, F32).reshape(-1, 4)


def lsd(gray_u8):
    """raw LSD output (x1, y1, x2, y2) float32, in detection order, of an 8-bit grey image"""
    scaled = resize_f64(blur(np.asarray(gray_u8, np.uint8)))
    return LSD(scaled).run()


# ---- host side: upscale, length filter, priority-queue order, cap -------------------------------------------------
def pq_order(lengths):
    """pop order of std::priority_queue<_, vector, less-on-length> after pushing `lengths` in order (libstdc++'s
    push_heap / pop_heap), as indices into `lengths`"""
    h = []
    for i, v in enumerate(lengths):
        h.append((v, i))
        hole = len(h) - 1
        while hole > 0:
            par = (hole - 1) // 2
            if not (h[par][0] < v):
                break
            h[hole] = h[par]
            hole = par
        h[hole] = (v, i)
    out = []
    while h:
        out.append(h[0][1])
        last = h.pop()
        n = len(h)
        if n == 0:
            break
        hole, second = 0, 0
        while second < (n - 1) // 2:
            second = 2 * (second + 1)
            if h[second][0] < h[second - 1][0]:
                second -= 1
            h[hole] = h[second]
            hole = second
        if (n & 1) == 0 and second == (n - 2) // 2:
            second = 2 * (second + 1)
            h[hole] = h[second - 1]
            hole = second - 1
        while hole > 0:
            par = (hole - 1) // 2
            if not (h[par][0] < last[0]):
                break
            h[hole] = h[par]
            hole = par
        h[hole] = last
    return out


def finish(raw, rows, cols, upx, upy, max_segments=3000):
    segs = raw.astype(F32).copy()
    segs[:, 0] *= upx
    segs[:, 1] *= upy
    segs[:, 2] *= upx
    segs[:, 3] *= upy
    dx = segs[:, 0] - segs[:, 2]
    dy = segs[:, 1] - segs[:, 3]
    length = np.sqrt(dx * dx + dy * dy).astype(F32)
    diag = np.sqrt(F32(rows * rows) + F32(cols * cols)).astype(F32)
    min_len = F32(diag * F32(0.005))
    keep = [i for i in range(len(segs)) if length[i] > min_len]
    order = pq_order([float(length[i]) for i in keep])
    return segs[[keep[i] for i in order]][:max_segments].reshape(-1, 4)


def detect(image, max_image_width=-1, max_segments=3000):
    image = np.asarray(image, np.uint8)
    g = gray_rgb(image) if image.ndim == 3 else image
    rows, cols = g.shape
    small, upx, upy = downscale(g, max_image_width)
    return finish(lsd(small), rows, cols, upx, upy, max_segments)


def stages(image, max_image_width=-1):
    """every stage of one image, as the GPU's stage hook reports them: gray, small (the image handed to LSD), blur,
    deg (float32 degrees, NOTDEF where undefined), mod, raw (LSD's output in detection order), seeds, nfa_evals,
    max_grad (-1: no gradient defined), upx / upy, and `walk`, the LSD object with its branch counters"""
    image = np.asarray(image, np.uint8)
    g = gray_rgb(image) if image.ndim == 3 else image
    small, upx, upy = downscale(g, max_image_width)
    b = blur(small)
    walk = LSD(resize_f64(b))
    raw = walk.run()
    return {"gray": g, "small": small, "blur": b, "deg": walk.deg, "mod": walk.mod, "raw": raw, "seeds": walk.seeds,
            "nfa_evals": walk.nfa_evals, "max_grad": walk.max_grad, "upx": upx, "upy": upy, "walk": walk}
