"""float64 reference of the EDI prior table (csrc/kernels_edi_prior.hip, evd_edi_prior): LLFFEventsDataset.compute_edi_prior
(data/loader_events.py:99-131) restated in this project's own formulation, with a first-order error bound E per element in units of
u = 2^-24: a float32 evaluation (the reference's numpy one, or the kernels') must satisfy |got - ref| <= K u E with K = 2.  Test
infrastructure only; also the seeded inputs of golden G36's 'flt' case, which the generator (tools/gen_golden.py) and the tests share.

Formulation.  With t the ascending timestamp column and b[i, 0..steps) the boundaries of image i (np.linspace in float64):
  left[i, j] = #{e: t_e < b[i, j]},  right[i, j] = #{e: t_e <= b[i, j]}
  window j of image i = the events with index in [left[i, j], right[i, j + 1])                       rule "closed" (the reference's, :119-121)
                                               [left[i, j], left[i, j + 1])                          rule "open_right": what an exclusive right edge would give
                                               [right[i, j], right[i, j + 1])                        rule "open_left": an exclusive left edge
  an event at (x, y): fx = floor(x), ax = x - fx; it puts (1 - ax) on column fx and, if ax > 0, ax on column fx + 1; rows alike; the weight of a
  tap is the product; a tap outside [0, w) x [0, h) is dropped -- on EVERY side (the kernels' rule; the reference lets a negative index wrap)
  Sp / Sn [j, pixel] = the sums of the tap weights of the window's positive / other events, Np / Nn the tap counts
  bii_j = c_pos Sp - c_neg Sn  with the thresholds as float32 values (the reference multiplies float32 planes by them, utils/edi.py:69)
  E_k = -(bii_k + ... + bii_(M-1)) for k < M = (steps - 1) / 2, 0 for k = M, bii_M + ... + bii_(k-1) for k > M;  s = sum_k exp(E_k)
  sharp = steps blurry / s, the same for the three channels
Error model (units of u; float32 evaluation):
  per window    a float32 plane summed tap by tap: N S;  the two products and the difference: 2 (c S) on the larger side
                A_j = c_pos Np Sp + c_neg Nn Sn + 2 (c_pos Sp + c_neg Sn)
  per exponent  its m windows summed one after the other: m - 1 roundings, each on at most sum |bii_j|
                B_k = sum_j A_j + (m - 1) sum_j |bii_j|
  the sum       exp conditions its argument's error by itself and rounds once: exp(E_k) (B_k + 1);  steps - 1 additions on at most s
                D = sum_k exp(E_k) (B_k + 1) + (steps - 1) s
  sharp         the product and the division: E = |sharp| (D / s + 2)
The fixed-point kernel sums its planes exactly (each weight within 2^-41 of the float64 one), so it has less rounding than this form."""
import numpy as np

U = 2.0 ** -24
K = 2.0
RULES = ("closed", "open_right", "open_left")


def windows(t, bounds):
    """-> left, right int64, the shape of bounds"""
    t = np.asarray(t, np.float64)
    return np.searchsorted(t, bounds, side="left").astype(np.int64), np.searchsorted(t, bounds, side="right").astype(np.int64)


def window_range(left_i, right_i, j, rule):
    if rule == "closed":
        return int(left_i[j]), int(right_i[j + 1])
    if rule == "open_right":
        return int(left_i[j]), int(left_i[j + 1])
    if rule == "open_left":
        return int(right_i[j]), int(right_i[j + 1])
    raise ValueError(rule)


def splat(x, y, h, w):
    """weight sum and tap count per pixel of the events at (x, y): two float64 [h w]"""
    S, Nt = np.zeros(h * w), np.zeros(h * w)
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    for dx, wx in ((0, 1.0 - ax), (1, ax)):
        for dy, wy in ((0, 1.0 - ay), (1, ay)):
            cx, cy = fx + dx, fy + dy
            ok = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
            if dx:
                ok &= ax > 0
            if dy:
                ok &= ay > 0
            idx = (cy[ok] * w + cx[ok]).astype(np.int64)
            S += np.bincount(idx, weights=(wx * wy)[ok], minlength=h * w)
            Nt += np.bincount(idx, minlength=h * w)
    return S, Nt


def edi_prior_ref(events, id_to_coords, tms_start, tms_end, images, steps, cpos, cneg, rule="closed"):
    """events [N, >= 3] (coordinate id, timestamp, polarity, ...), id_to_coords [Ncoords, 2], images [n, H, W, 3] ->
    dict(prior [n, H, W, 3] float64, E the same shape (units of u), left, right [n, steps] int64)"""
    ev = np.asarray(events, np.float64)
    i2c = np.asarray(id_to_coords, np.float64)
    img = np.asarray(images, np.float64)
    n, h, w, _ = img.shape
    cp, cn = float(np.float32(cpos)), float(np.float32(cneg))
    bounds = np.stack([np.linspace(a, b, steps) for a, b in zip(np.asarray(tms_start, np.float64), np.asarray(tms_end, np.float64))])
    left, right = windows(ev[:, 1], bounds)
    M = (steps - 1) // 2
    prior, E = np.zeros_like(img), np.zeros_like(img)
    for i in range(n):
        bii, A = np.zeros((steps - 1, h * w)), np.zeros((steps - 1, h * w))
        for j in range(steps - 1):
            lo, hi = window_range(left[i], right[i], j, rule)
            e = ev[lo:hi]
            xy = i2c[e[:, 0].astype(np.int64)]
            pos = e[:, 2] > 0
            Sp, Np = splat(xy[pos, 0], xy[pos, 1], h, w)
            Sn, Nn = splat(xy[~pos, 0], xy[~pos, 1], h, w)
            bii[j] = cp * Sp - cn * Sn
            A[j] = cp * Np * Sp + cn * Nn * Sn + 2.0 * (cp * Sp + cn * Sn)
        s, D = np.zeros(h * w), np.zeros(h * w)
        for k in range(steps):
            js = slice(k, M) if k < M else slice(M, k)
            m = js.stop - js.start
            Ek = (-1.0 if k < M else 1.0) * bii[js].sum(0)
            Bk = A[js].sum(0) + max(m - 1, 0) * np.abs(bii[js]).sum(0)
            ex = np.exp(Ek)
            s += ex
            D += ex * (Bk + 1.0)
        D += (steps - 1) * s
        prior[i] = (steps * img[i].reshape(h * w, 3) / s[:, None]).reshape(h, w, 3)
        E[i] = np.abs(prior[i]) * (D / s + 2.0).reshape(h, w, 1)
    return {"prior": prior, "E": E, "left": left, "right": right}


def worst_ratio(got, ref, E):
    """max |got - ref| / (u E) (E = 0 only where ref = 0: there any difference counts as inf)"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / (U * E))
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------ golden G36, case 'flt': seeded inputs
G36_FLT_ROWS = 8            # channels 1 and 2 of the 'flt' result are stored on every 8th row


def g36_flt_inputs():
    """Two exposures on the DAVIS frame (260 x 346), steps 9, 120 000 events with rectified float32 coordinates: a uniform part over the right /
    lower 45 % of the frame (the rest stays silent, as most of a real frame does), a clustered part that piles dozens of taps per window on a
    few pixels, coordinates in the last column / row whose ceil tap falls outside, and none below 0.  Images: 8-bit values / 255."""
    rs = np.random.RandomState(3601)
    h, w, steps, n_ev, n_coords = 260, 346, 9, 120_000, 30_000
    cx = rs.uniform(0.3 * w, w - 0.01, n_coords)
    cy = rs.uniform(0.35 * h, h - 0.01, n_coords)
    cx[:200] = rs.uniform(w - 1, w - 0.01, 200)               # ceil tap off the right edge
    cy[200:400] = rs.uniform(h - 1, h - 0.01, 200)            # ... off the bottom edge
    cx[400:420] = w - 1                                        # exactly the last column / row
    cy[420:440] = h - 1
    cx[440:460] = np.floor(cx[440:460])                        # integer coordinates inside
    cy[450:470] = np.floor(cy[450:470])
    hot = np.arange(1000, 1040)                                # 40 coordinates around three spots: the clusters
    spots = np.array([[150.3, 120.6], [300.8, 200.2], [222.5, 181.5]])
    cx[hot] = spots[rs.randint(0, 3, 40), 0] + rs.uniform(-0.6, 0.6, 40)
    cy[hot] = spots[rs.randint(0, 3, 40), 1] + rs.uniform(-0.6, 0.6, 40)
    i2c = np.stack([cx, cy], -1).astype(np.float32).astype(np.float64)
    ids = rs.randint(0, n_coords, n_ev)
    clustered = rs.rand(n_ev) < 0.08
    ids[clustered] = hot[rs.randint(0, 40, int(clustered.sum()))]
    start = np.array([1_000_000.0, 1_040_000.0])
    end = start + np.array([24_000.0, 30_000.0])
    t = np.sort(rs.randint(995_000, 1_075_000, n_ev)).astype(np.float64)
    p = np.where(rs.rand(n_ev) < 0.55, 1.0, -1.0)
    events = np.stack([ids.astype(np.float64), t, p, np.zeros(n_ev)], -1)
    images = (rs.randint(13, 256, (2, h, w, 3)) / 255.0).astype(np.float32)
    return {"events": events, "id_to_coords": i2c, "tms_start": start, "tms_end": end, "images": images, "steps": steps, "cpos": 0.21, "cneg": 0.26}
