"""Exact reference of the cloth rasterisers (gym_cloth_amd/csrc/cloth_render.hpp: k_render; cloth_render_obs.hpp: k_render_obs).

TEST INFRASTRUCTURE, NOT PRODUCT CODE (only tests/ import it). oracle/render_oracle.py restates the kernels' float32 expressions and so
pins their BITS; this file states the RULES geometrically and computes them exactly, so a wrong rule written alike in the kernel and in
the restatement does not pass here. Its inputs are the float32 numbers the device receives -- the positions a handle holds, cast to
float32 as the kernels cast them, and the float32 scene (camera, rotation, fx = fl32(fl32(lens / sensor) * W), cx = fl32(W / 2),
cy = fl32(H / 2), colours, lamp) -- which are dyadic rationals: everything geometric below is integer arithmetic on them over one power
of two. A float64 pass decides what it can decide with certainty and hands the rest (centres on or next to an edge, near-equal depths)
to the integers.

The rules
  faces       per grid cell pp = r N + c: [pp, pp + N, pp + 1] and [pp + 1, pp + N, pp + N + 1]
  projection  camera space R (p - cam), depth d = -z_cam; a face with a vertex at d <= fl32(1e-6) draws nothing;
              u = fx x_cam / d + cx, v = cy - fy y_cam / d. A vertex is kept homogeneous, (u d, v d, d): no division.
  coverage    the pixel centre (ix + 1/2, iy + 1/2) strictly inside the face; a centre ON an edge is covered iff the point
              (x + eps, y + eps^2), eps -> 0+, is inside -- the top-left rule in image coordinates (y down): a left edge owns its
              centres, a horizontal edge owns them if it is a top edge. The sign of an edge function is the sign of the 3x3 determinant
              of two homogeneous vertices and (x, y, 1) (all d > 0). Zero-area faces cover nothing.
  depth       1 / d of the face's plane at the centre: with lambda the solution of sum lambda_i (u_i d_i, v_i d_i, d_i) = (x, y, 1)
              (Cramer: lambda_i = E_i / A, the determinants above), 1 / d = sum lambda_i. The nearest covering face wins. An uncovered
              pixel reports cam[2] (the bed plane) and the background bytes.
  side        the front colour shows iff the projected face has negative signed area in image coordinates, XOR the swap flag
  colour      vertex normal = sum of the incident faces' unnormalised cross products (exact integers); I_v = ambient + energy |n . L| / |n|
              (lambert 0 where n = 0); pixel intensity = the screen-space barycentric mix sum b_i I_i, b_i = lambda_i d_i;
              byte = floor(clamp(col I, 0, 1) 255 + 1/2). |n| is the one inexact step: float64, its 2^-53 carried in the bound.

What float32 may legitimately decide otherwise -- the bounds, DERIVED (u = 2^-24 the unit roundoff; first order, times SAFETY = 2 for the
second-order terms; every magnitude is the exact value's), never measured:
  vertex      X = p - cam: u |X| per component. x_c = R0 X + R1 Y + R2 Z: one rounding in X, one in the product, two in the sums:
              dx_c <= 4 u (|R0 X| + |R1 Y| + |R2 Z|); d alike. q = (fx x_c) / d: dq <= |fx| dx_c / d + |q| (dd / d + 2 u).
              u_pix = q + cx: du <= dq + u |u_pix|; dv alike.
  edge        e = (x2 - x1)(py - y1) - (y2 - y1)(px - x1) =: a g - c h (px, py exact): da <= dx1 + dx2 + u |a|, dg <= dy1 + u |g|,
              d(a g) <= |a| dg + |g| da + u |a g|, c h alike, de <= d(a g) + d(c h) + u (|a g| + |c h|). The area is the edge function of
              (v0, v1) at v2 with dg <= dy0 + dy2 + u |g| (both ends inexact). tau = SAFETY de is the EDGE-DISTANCE THRESHOLD in edge-function
              units (a distance of tau / |edge| pixels).
  coverage    a (face, centre) pair is certain if every s e_i > tau_i (inside) or one s e_i < -tau_i (outside), s the area's sign; where
              |area| <= tau_area the sign itself is open: outside is then certain only if one e_i > tau_i and another e_j < -tau_j. Every
              pair that is not certain makes its pixel `ambiguous`.
  depth       b_i = e_i / A: db_i <= (de_i + |b_i| dA) / |A| + u |b_i|; 1 / d_i: relative dd_i / d_i + u;
              d(sum b_i / d_i) <= sum [db_i / d_i + (|b_i| / d_i)(dd_i / d_i + 2 u)] + 2 u sum |b_i| / d_i; the reported depth is one more
              division: rho = SAFETY d(1/d) d + 2 u is the RELATIVE DEPTH BOUND of the pair. A pixel is ambiguous if another covering face
              could win in float32 (its 1 / d (1 + rho') reaches the winner's 1 / d (1 - rho)) and shows other bytes or the other side; if it
              shows the same, the pixel's depth bound widens by that face's distance and bound.
  colour      normal component k: the two differences (u each), two products, one subtraction per face and <= 6 additions:
              dn_k <= 10 u S_k, S_k the sum of the |products|. |n|: d|n| <= |dn| + 3 u |n|. lambert: dl <= (sum |L_k| (dn_k + 3 u |n_k|)
              + l (|dn| + 3 u |n|)) / |n| + 2 u l, at most 1. I_v: dI_v <= energy dl + 2 u I_v. Pixel: dI <= sum (db_i I_i + |b_i| dI_i)
              + 3 u sum |b_i| I_i; t = clamp(col I) 255 + 1/2: dt <= SAFETY (255 col dI + 4 u t) + 1e-9 (the reference's own float64).
              The byte may be floor(t - dt) .. floor(t + dt) -- inside the WINDOW around a quantisation step either neighbour, outside it the
              reference's byte -- and never differs from floor(t) by more than 1; a pixel with dt > 1/2 is ambiguous.
  1e-6        a vertex whose exact d is within SAFETY dd of fl32(1e-6) is refused (ValueError): the states keep away from it.

States marked exact: the reference proves from its exact values that float32 computes them without rounding -- every step of the
projection, every difference and product of every edge function and area over the face's bounding box, and on covered pixels the
barycentric quotients, 1 / d_i, their products and sums -- and raises if one is not representable. Then tau = rho = 0: no pixel is
geometrically ambiguous, the depth is the exact d to the bit, and (asserted too) no colour window holds a quantisation step, so every byte
is compared for equality.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

F = np.float32
U32 = 2.0 ** -24
SAFETY = 2.0
D_MIN = Fraction(float(F(1e-6)))

Scene = namedtuple("Scene", "W H cam R fx fy cx cy front back bg light ambient energy")

Exact = namedtuple("Exact", "W H covered face front inv_d depth depth_bound t t_err byte other_side_differs ambiguous on_outline "
                            "face_v n_near_edge n_depth_close exact")


def scene(width, height, cam_pos, world_to_cam, lens_mm, sensor_mm, front, back, background, light_dir, ambient, energy):
    """The float32 scene values the device receives (api_observe.hip: fill_scene)."""
    W, H = int(width), int(height)
    fx = F(F(lens_mm) / F(sensor_mm)) * F(W)
    f3 = lambda v: np.asarray(v, dtype=F).reshape(3)
    return Scene(W, H, f3(cam_pos), np.asarray(world_to_cam, dtype=F).reshape(9), F(fx), F(fx), F(0.5) * F(W), F(0.5) * F(H),
                 f3(front), f3(back), f3(background), f3(light_dir), F(ambient), F(energy))


def faces(n_side):
    N = int(n_side)
    out = []
    for r in range(N - 1):
        for c in range(N - 1):
            pp = r * N + c
            out.append((pp, pp + N, pp + 1))
            out.append((pp + 1, pp + N, pp + N + 1))
    return out


def border_edges(n_side):
    """{(face, k)}: edge k (opposite the face's k-th vertex) of that face lies on the grid's border, i.e. belongs to no other face."""
    N = int(n_side)
    out = set()
    for r in range(N - 1):
        for c in range(N - 1):
            t = 2 * (r * (N - 1) + c)
            if r == 0: out.add((t, 1))            # (pp + 1, pp)
            if c == 0: out.add((t, 2))            # (pp, pp + N)
            if r == N - 2: out.add((t + 1, 0))    # (pp + N, pp + N + 1)
            if c == N - 2: out.add((t + 1, 1))    # (pp + N + 1, pp + 1)
    return out


def _ints(values):
    """float array -> (list of ints, shift): values[i] == ints[i] / 2**shift exactly."""
    ratios = [float(v).as_integer_ratio() for v in np.asarray(values, dtype=np.float64).reshape(-1)]
    shift = max([d.bit_length() - 1 for _, d in ratios] + [0])
    return [n * ((1 << shift) // d) for n, d in ratios], shift


def f32_ok(n, shift):
    """Is the rational n / 2**shift a (normal) float32?"""
    if n == 0:
        return True
    n = abs(n)
    tz = (n & -n).bit_length() - 1
    m = n >> tz
    return m.bit_length() <= 24 and tz - shift >= -126 and tz - shift + m.bit_length() - 1 <= 127


def _frac_ok(q):
    q = Fraction(q)
    den = q.denominator
    return den & (den - 1) == 0 and f32_ok(q.numerator, den.bit_length() - 1)


def _det3(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))


def _q8(t):
    return np.floor(t).astype(np.int64)


class NotExact(AssertionError):
    """A state marked exact has a float32 step that rounds."""


def render(pos, n_side, sc, swap=False, exact=False):
    """pos [P, 3] (cast to float32 as the kernels do), sc: scene(...). -> Exact, per pixel [H, W]:
      covered, face (winning face index, -1), front (the side shown), inv_d (object array of Fractions, None where uncovered),
      depth (float64 of the exact depth; cam[2] where uncovered), depth_bound (relative), t [H, W, 3] (clamp(col I) 255 + 1/2; floor(t) is
      the byte), t_err, byte (uint8), other_side_differs (the other side's bytes would differ: the side is observable), ambiguous,
      on_outline (the centre lies exactly on a border edge of the grid, within the edge); face_v [faces, 2]: min and max image y of every
      face that is drawn and has an area (nan for the others); n_near_edge / n_depth_close: ambiguous pixels by
      cause; exact: the flag it was called with (and proved)."""
    N, P, W, H = int(n_side), int(n_side) ** 2, sc.W, sc.H
    w32 = np.asarray(pos).astype(F).astype(np.float64)
    assert w32.shape == (P, 3) and np.isfinite(w32).all()
    tri = faces(N)
    nF = len(tri)
    tri_a = np.array(tri, dtype=np.int64)
    # ---- exact vertices: homogeneous (U, V, D) over 2**T ----------------------------------------------------------------------------
    pw, s = _ints(np.concatenate([w32.reshape(-1), sc.cam.astype(np.float64)]))
    cam_i = pw[3 * P:]
    Ri, r = _ints(sc.R)
    (fxi, cxi, cyi), f = _ints([sc.fx, sc.cx, sc.cy])
    T = s + r + f
    hv, cs = [], []                                   # homogeneous vertex, camera-space (xc, yc, d) over 2**(s + r)
    for i in range(P):
        X, Y, Z = pw[3 * i] - cam_i[0], pw[3 * i + 1] - cam_i[1], pw[3 * i + 2] - cam_i[2]
        xc = Ri[0] * X + Ri[1] * Y + Ri[2] * Z
        yc = Ri[3] * X + Ri[4] * Y + Ri[5] * Z
        d = -(Ri[6] * X + Ri[7] * Y + Ri[8] * Z)
        hv.append((fxi * xc + cxi * d, cyi * d - fxi * yc, d << f))
        cs.append((xc, yc, d))
    dmin_i = D_MIN * (1 << (s + r))
    ok_v = np.array([c[2] > dmin_i for c in cs])      # d > fl32(1e-6), exactly
    # float64 views and the per-vertex float32 error of (u, v, d)
    Rf, camf = sc.R.astype(np.float64), sc.cam.astype(np.float64)
    Xf = w32 - camf[None, :]
    Sx = np.abs(Xf * Rf[None, 0:3]).sum(axis=1); Sy = np.abs(Xf * Rf[None, 3:6]).sum(axis=1); Sd = np.abs(Xf * Rf[None, 6:9]).sum(axis=1)
    xcf = np.array([c[0] / (1 << (s + r)) for c in cs]); ycf = np.array([c[1] / (1 << (s + r)) for c in cs])
    df = np.array([c[2] / (1 << (s + r)) for c in cs])
    dd = 4 * U32 * Sd
    near = np.abs(df - float(D_MIN)) <= SAFETY * dd + 1e-30
    if near.any() and not exact:
        raise ValueError("a vertex has d within the float32 error of 1e-6: the drop rule is a coin toss")
    ds = np.where(ok_v, df, 1.0)
    uf = np.where(ok_v, [h[0] / h[2] if h[2] > 0 else 0.0 for h in hv], 0.0)
    vf = np.where(ok_v, [h[1] / h[2] if h[2] > 0 else 0.0 for h in hv], 0.0)
    fxf = float(sc.fx)
    qx, qy = fxf * xcf / ds, fxf * ycf / ds
    du = fxf * 4 * U32 * Sx / ds + np.abs(qx) * (dd / ds + 2 * U32) + U32 * np.abs(uf)
    dv = fxf * 4 * U32 * Sy / ds + np.abs(qy) * (dd / ds + 2 * U32) + U32 * np.abs(vf)
    if exact:
        du = np.zeros(P); dv = np.zeros(P); dd = np.zeros(P)
        _prove_vertices_exact(pw, cam_i, Ri, fxi, cxi, cyi, s, r, f, P, ok_v, hv)
    # ---- vertex intensities ----------------------------------------------------------------------------------------------------------
    Iv, dIv = _intensities(w32, pw, s, N, tri, sc, exact)
    # ---- faces --------------------------------------------------------------------------------------------------------------------
    drawn = ok_v[tri_a].all(axis=1)
    A_i = [(_det3(hv[a], hv[b], hv[c]) if drawn[t] else 0) for t, (a, b, c) in enumerate(tri)]
    sgn = np.array([(A > 0) - (A < 0) for A in A_i], dtype=np.float64)
    x = uf[tri_a]; y = vf[tri_a]; dx = du[tri_a]; dy = dv[tri_a]                                   # [nF, 3]
    pad = 1e-3
    mnx, mxx = x.min(axis=1) - dx.max(axis=1) - pad, x.max(axis=1) + dx.max(axis=1) + pad
    mny, mxy = y.min(axis=1) - dy.max(axis=1) - pad, y.max(axis=1) + dy.max(axis=1) + pad
    ix0 = np.clip(np.ceil(mnx - 0.5), 0, W).astype(np.int64); ix1 = np.clip(np.floor(mxx - 0.5), -1, W - 1).astype(np.int64)
    iy0 = np.clip(np.ceil(mny - 0.5), 0, H).astype(np.int64); iy1 = np.clip(np.floor(mxy - 0.5), -1, H - 1).astype(np.int64)
    fl, pxl, pyl = [], [], []
    for t in np.nonzero(drawn & (ix1 >= ix0) & (iy1 >= iy0))[0]:
        gx, gy = np.meshgrid(np.arange(ix0[t], ix1[t] + 1), np.arange(iy0[t], iy1[t] + 1))
        fl.append(np.full(gx.size, t, dtype=np.int64)); pxl.append(gx.reshape(-1)); pyl.append(gy.reshape(-1))
    covered = np.zeros((H, W), dtype=bool); face = np.full((H, W), -1, dtype=np.int64); front = np.zeros((H, W), dtype=bool)
    inv_d = np.full((H, W), None, dtype=object); depth = np.full((H, W), float(sc.cam[2])); depth_bound = np.zeros((H, W))
    bgt = np.minimum(np.maximum(sc.bg.astype(np.float64), 0.0), 1.0) * 255.0 + 0.5
    t_out = np.tile(bgt, (H, W, 1)); t_err = np.zeros((H, W)); other = np.zeros((H, W), dtype=bool)
    amb_edge = np.zeros((H, W), dtype=bool); amb_depth = np.zeros((H, W), dtype=bool); amb_col = np.zeros((H, W), dtype=bool)
    on_outline = np.zeros((H, W), dtype=bool)
    if fl:
        fi = np.concatenate(fl); pix = np.concatenate(pxl); piy = np.concatenate(pyl)
        px, py = pix + 0.5, piy + 0.5
        e = np.empty((3, len(fi))); de = np.empty((3, len(fi)))
        for k, (i1, i2) in enumerate(((1, 2), (2, 0), (0, 1))):                                 # edge k is opposite vertex k
            x1, y1, x2, y2 = x[fi, i1], y[fi, i1], x[fi, i2], y[fi, i2]
            e[k], de[k] = _edge(x1, y1, x2, y2, px, py, dx[fi, i1], dy[fi, i1], dx[fi, i2], dy[fi, i2], 0.0, 0.0)
        Af, dAf = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2], dx[:, 0], dy[:, 0], dx[:, 1], dy[:, 1], dx[:, 2], dy[:, 2])
        sf = sgn[fi]
        se = sf[None, :] * e
        eps64 = 1e-12 * (np.abs(x[fi]).max(axis=1) + np.abs(y[fi]).max(axis=1) + W + H + 1.0) ** 2
        sure_in = (se > eps64).all(axis=0) & (sf != 0)
        sure_out = (se < -eps64).any(axis=0) | (sf == 0)
        inside = sure_in.copy()
        border = border_edges(N)
        for j in np.nonzero(~sure_in & ~sure_out)[0]:                                           # the integers decide
            t = int(fi[j]); a, b, c = tri[t]
            p = (2 * int(pix[j]) + 1, 2 * int(piy[j]) + 1, 2)
            sg = int(sgn[t])
            ins, closed = True, True
            zero = []
            for k, (v1, v2) in enumerate(((b, c), (c, a), (a, b))):
                E = sg * _det3(hv[v1], hv[v2], p)
                if E < 0:
                    ins = closed = False
                elif E == 0:
                    zero.append(k)
                    P1, P2 = hv[v1], hv[v2]
                    gx, gy = sg * (P1[1] * P2[2] - P1[2] * P2[1]), -sg * (P1[0] * P2[2] - P1[2] * P2[0])   # d e / d x, d e / d y (times d1 d2 > 0)
                    if not (gx > 0 or (gx == 0 and gy > 0)):                                    # (x + eps, y + eps^2) is not inside
                        ins = False
            inside[j] = ins
            if closed and any((t, k) in border for k in zero):
                on_outline[piy[j], pix[j]] = True
        # what float32 may decide otherwise
        tau = SAFETY * de
        tauA = SAFETY * dAf[fi]
        area_open = np.abs(Af[fi]) <= tauA
        pos_c, neg_c = se > tau, se < -tau
        if exact:
            certain = np.ones(len(fi), dtype=bool)
            _prove_edges_exact(hv, tri, fi, pix, piy)
        else:
            certain = np.where(area_open, (e > tau).any(axis=0) & (e < -tau).any(axis=0), pos_c.all(axis=0) | neg_c.any(axis=0))
        np.logical_or.at(amb_edge, (piy[~certain], pix[~certain]), True)
        # ---- covering pairs: depth, side, colour ---------------------------------------------------------------------------------------
        j = np.nonzero(inside)[0]
        if len(j):
            fj, xj, yj = fi[j], pix[j], piy[j]
            Aj = Af[fj]
            b = e[:, j] / Aj[None, :]                                                           # screen-space barycentrics, float64
            db = (de[:, j] + np.abs(b) * dAf[fj][None, :]) / np.abs(Aj)[None, :] + U32 * np.abs(b)
            dvert = df[tri_a[fj]].T                                                             # [3, n] vertex depths
            ddv = dd[tri_a[fj]].T
            iw = 1.0 / dvert
            invd = (b * iw).sum(axis=0)
            dinv = (db * iw + np.abs(b) * iw * (ddv / dvert + 2 * U32)).sum(axis=0) + 2 * U32 * (np.abs(b) * iw).sum(axis=0)
            rho = np.zeros(len(j)) if exact else SAFETY * dinv / invd + 2 * U32
            Ivj, dIvj = Iv[tri_a[fj]].T, dIv[tri_a[fj]].T
            I = (b * Ivj).sum(axis=0)
            dI = (db * Ivj + np.abs(b) * dIvj).sum(axis=0) + 3 * U32 * (np.abs(b) * Ivj).sum(axis=0)
            if exact:
                dI = (np.abs(b) * dIvj).sum(axis=0) + 3 * U32 * (np.abs(b) * Ivj).sum(axis=0)
            is_front = (sgn[fj] < 0) != bool(swap)
            colf, colb = sc.front.astype(np.float64), sc.back.astype(np.float64)
            col = np.where(is_front[:, None], colf[None, :], colb[None, :])
            col_o = np.where(is_front[:, None], colb[None, :], colf[None, :])
            tt = np.clip(col * I[:, None], 0.0, 1.0) * 255.0 + 0.5
            tt_o = np.clip(col_o * I[:, None], 0.0, 1.0) * 255.0 + 0.5
            dt = SAFETY * (255.0 * col.max(axis=1) * dI + 4 * U32 * tt.max(axis=1)) + 1e-9
            byt = _q8(tt)
            # the winner of each pixel: float64 order, the integers where two are close
            lin = yj * W + xj
            order = np.lexsort((invd, lin))
            lin_s = lin[order]
            last = np.r_[lin_s[1:] != lin_s[:-1], True]
            start = np.r_[True, lin_s[1:] != lin_s[:-1]]
            starts = np.nonzero(start)[0]; ends = np.nonzero(last)[0]
            for s0, e0 in zip(starts, ends):
                grp = order[s0:e0 + 1]
                win = grp[-1]
                if len(grp) > 1:
                    close = [g for g in grp[:-1] if invd[g] >= invd[win] * (1 - 1e-11)]
                    if close:                                                                   # exact comparison
                        ex = {g: _inv_d_exact(hv, tri[int(fj[g])], int(xj[g]), int(yj[g]), T) for g in close + [win]}
                        win = max(ex, key=lambda g: (ex[g], tuple(byt[g])))
                    for g in grp:
                        if g == win:
                            continue
                        if invd[g] * (1 + rho[g]) >= invd[win] * (1 - rho[win]) or exact and invd[g] == invd[win]:
                            if (byt[g] != byt[win]).any() or is_front[g] != is_front[win] or dt[g] > 0.5:
                                amb_depth[yj[win], xj[win]] = True
                            else:
                                rho[win] = rho[win] + rho[g] + abs(invd[g] / invd[win] - 1.0)
                yy, xx = int(yj[win]), int(xj[win])
                covered[yy, xx] = True; face[yy, xx] = fj[win]; front[yy, xx] = is_front[win]
                q = _inv_d_exact(hv, tri[int(fj[win])], xx, yy, T)
                inv_d[yy, xx] = q; depth[yy, xx] = float(1 / q); depth_bound[yy, xx] = rho[win]
                t_out[yy, xx] = tt[win]; t_err[yy, xx] = dt[win]; other[yy, xx] = (_q8(tt_o[win]) != byt[win]).any()
                if dt[win] > 0.5:
                    amb_col[yy, xx] = True
                if exact:
                    _prove_depth_exact(hv, tri[int(fj[win])], xx, yy, T, q)
    byte = _q8(t_out).astype(np.uint8)
    ambiguous = amb_edge | amb_depth | amb_col
    if exact:
        straddle = covered & ((np.floor(t_out - t_err[..., None]) != np.floor(t_out + t_err[..., None])).any(axis=-1))
        if ambiguous.any() or straddle.any():
            raise NotExact("exact state with %d ambiguous pixels, %d colour windows on a quantisation step" % (ambiguous.sum(), straddle.sum()))
    live = drawn & (sgn != 0)
    face_v = np.where(live[:, None], np.stack([y.min(axis=1), y.max(axis=1)], axis=1), np.nan)
    return Exact(W, H, covered, face, front, inv_d, depth, depth_bound, t_out, t_err, byte, other, ambiguous, on_outline, face_v,
                 int(amb_edge.sum()), int((amb_depth | amb_col).sum()), bool(exact))


def _edge(x1, y1, x2, y2, px, py, dx1, dy1, dx2, dy2, dpx, dpy):
    """Edge function of (v1 -> v2) at p in float64 and its float32 error bound (module docstring: edge)."""
    a, g, c, h = x2 - x1, py - y1, y2 - y1, px - x1
    da = dx1 + dx2 + U32 * np.abs(a); dc = dy1 + dy2 + U32 * np.abs(c)
    dg = dy1 + dpy + U32 * np.abs(g); dh = dx1 + dpx + U32 * np.abs(h)
    ag, ch = a * g, c * h
    de = (np.abs(a) * dg + np.abs(g) * da + U32 * np.abs(ag)) + (np.abs(c) * dh + np.abs(h) * dc + U32 * np.abs(ch)) + U32 * (np.abs(ag) + np.abs(ch))
    return ag - ch, de


def _inv_d_exact(hv, f, ix, iy, T):
    """1 / d of face f's plane at the centre of pixel (ix, iy): sum of the Cramer weights (module docstring: depth)."""
    a, b, c = f
    p = (2 * ix + 1, 2 * iy + 1, 2)
    E = _det3(hv[b], hv[c], p) + _det3(hv[c], hv[a], p) + _det3(hv[a], hv[b], p)          # 2**(2T + 1) times the true sum
    return Fraction(E << T, 2 * _det3(hv[a], hv[b], hv[c]))                                 # the area carries 2**(3T)


def _intensities(w32, pw, s, N, tri, sc, exact):
    """Per vertex: I_v in float64 and its float32 error bound (module docstring: colour)."""
    P = N * N
    n = [[0, 0, 0] for _ in range(P)]
    S = np.zeros((P, 3))
    for a, b, c in tri:
        ux, uy, uz = (pw[3 * b + k] - pw[3 * a + k] for k in range(3))
        tx, ty, tz = (pw[3 * c + k] - pw[3 * a + k] for k in range(3))
        cr = (uy * tz - uz * ty, uz * tx - ux * tz, ux * ty - uy * tx)
        ab = (abs(uy * tz) + abs(uz * ty), abs(uz * tx) + abs(ux * tz), abs(ux * ty) + abs(uy * tx))
        for v in (a, b, c):
            for k in range(3):
                n[v][k] += cr[k]
            S[v] += [float(Fraction(q, 1 << (2 * s))) for q in ab]
    Li, ls = _ints(sc.light)
    L = np.abs(sc.light.astype(np.float64))
    amb, en = float(sc.ambient), float(sc.energy)
    Iv, dIv = np.empty(P), np.empty(P)
    for v in range(P):
        n2 = n[v][0] ** 2 + n[v][1] ** 2 + n[v][2] ** 2
        dn = 10 * U32 * S[v]
        if n2 == 0:
            lam, dl = 0.0, (1.0 if S[v].any() else 0.0)          # float32 sums exact zeros to zero; anything else may leave a direction
        else:
            nn = math.sqrt(Fraction(n2, 1 << (4 * s)))
            dot = abs(n[v][0] * Li[0] + n[v][1] * Li[1] + n[v][2] * Li[2])
            lam = float(Fraction(dot, 1 << (2 * s + ls))) / nn
            nk = np.array([abs(float(Fraction(q, 1 << (2 * s)))) for q in n[v]])
            dnn = math.sqrt((dn ** 2).sum()) + 3 * U32 * nn
            dl = min(1.0, ((L * (dn + 3 * U32 * nk)).sum() + lam * dnn) / nn + 2 * U32 * lam)
        Iv[v] = amb + en * lam
        dIv[v] = abs(en) * dl + 2 * U32 * abs(Iv[v])
    return Iv, dIv


# ---- the proofs of the exact states ------------------------------------------------------------------------------------------------
def _need(ok, what):
    if not ok:
        raise NotExact("not float32-representable: " + what)


def _prove_vertices_exact(pw, cam_i, Ri, fxi, cxi, cyi, s, r, f, P, ok_v, hv):
    """Every step of the projection of every drawn vertex is a float32 (so float32 arithmetic, correctly rounded, computes it exactly)."""
    for i in range(P):
        X = [pw[3 * i + k] - cam_i[k] for k in range(3)]
        for k in range(3):
            _need(f32_ok(X[k], s), "p - cam")
        rows = []
        for row in range(3):
            acc = 0
            for k in range(3):
                pr = Ri[3 * row + k] * X[k]
                _need(f32_ok(pr, s + r), "R X")
                acc += pr
                _need(f32_ok(acc, s + r), "R X sum")
            rows.append(acc)
        if not ok_v[i]:
            continue
        d = -rows[2]
        for val, c0, sign in ((rows[0], cxi, 1), (rows[1], cyi, -1)):
            num = fxi * val
            _need(f32_ok(num, s + r + f), "fx x_c")
            q = Fraction(num, d << f)                            # (fx x_c) / d
            _need(_frac_ok(q), "(fx x_c) / d")
            _need(_frac_ok(Fraction(c0, 1 << f) + sign * q), "pixel coordinate")


def _prove_edges_exact(hv, tri, fi, pix, piy):
    """Every difference and product of every edge function, and of the area, over each face's bounding box."""
    cache = {}
    for j in range(len(fi)):
        t = int(fi[j])
        if t not in cache:
            v = [(Fraction(hv[q][0], hv[q][2]), Fraction(hv[q][1], hv[q][2])) for q in tri[t]]
            (x0, y0), (x1, y1), (x2, y2) = v
            for q in ((x1 - x0), (y2 - y0), (y1 - y0), (x2 - x0), (x1 - x0) * (y2 - y0), (y1 - y0) * (x2 - x0),
                      (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)):
                _need(_frac_ok(q), "area")
            cache[t] = v
        v = cache[t]
        px, py = Fraction(2 * int(pix[j]) + 1, 2), Fraction(2 * int(piy[j]) + 1, 2)
        for (x1, y1), (x2, y2) in ((v[1], v[2]), (v[2], v[0]), (v[0], v[1])):
            a, g, c, h = x2 - x1, py - y1, y2 - y1, px - x1
            for q in (a, g, c, h, a * g, c * h, a * g - c * h):
                _need(_frac_ok(q), "edge function")


def _prove_depth_exact(hv, f, ix, iy, T, inv_d):
    """On a covered pixel: the barycentric quotients, 1 / d_i, their products, the running sum and the final reciprocal."""
    a, b, c = f
    p = (2 * ix + 1, 2 * iy + 1, 2)
    A = _det3(hv[a], hv[b], hv[c])
    acc = Fraction(0)
    for (v1, v2), vk in (((b, c), a), ((c, a), b), ((a, b), c)):
        lam = Fraction(_det3(hv[v1], hv[v2], p) << T, 2 * A)          # the Cramer weight; b_k = lam d_k
        dk = Fraction(hv[vk][2], 1 << T)
        _need(_frac_ok(lam * dk), "barycentric quotient")
        _need(_frac_ok(1 / dk), "1 / d of a vertex")
        _need(_frac_ok(lam), "b / d")
        acc += lam
        _need(_frac_ok(acc), "sum b / d")
    assert acc == inv_d
    _need(_frac_ok(1 / inv_d), "depth")


# ---- the comparison every test goes through ----------------------------------------------------------------------------------------
def compare(ex, rgb, depth, bg_byte, tag="", stats=None):
    """One image of a rasteriser (rgb uint8 [H, W, 3], depth float32 [H, W] or None) against the reference `ex`: on every unambiguous
    pixel coverage (told by the background bytes, which no cloth pixel of these scenes shows), side and colour (the byte inside its window,
    never more than 1 from the reference's), depth within its bound -- in an exact state every byte and every depth bit. Raises
    AssertionError with the count and the first offenders; returns / updates the measured maxima."""
    stats = {} if stats is None else stats
    ok = ~ex.ambiguous
    bg = np.asarray(bg_byte, dtype=np.uint8)
    assert not (ex.byte[ex.covered & ok] == bg).all(axis=-1).any(), (tag, "a cloth pixel shows the background bytes: coverage is not observable")
    got_cov = (rgb != bg).any(axis=-1)

    def fail(mask, what):
        ys, xs = np.nonzero(mask)
        raise AssertionError("%s: %s at %d pixels, first (x, y): %s" % (tag, what, len(ys), list(zip(xs[:6].tolist(), ys[:6].tolist()))))

    if ((got_cov != ex.covered) & ok).any():
        fail((got_cov != ex.covered) & ok, "coverage differs")
    m = ok & ex.covered
    lo = np.floor(ex.t - ex.t_err[..., None]); hi = np.floor(ex.t + ex.t_err[..., None])
    g = rgb.astype(np.float64)
    bad = m & ((g < lo) | (g > hi) | (np.abs(g - ex.byte) > 1)).any(axis=-1)
    if bad.any():
        fail(bad, "bytes outside their window")
    stats["bytes_off_by_one"] = stats.get("bytes_off_by_one", 0) + int((m[..., None] & (rgb != ex.byte)).sum())
    if depth is not None:
        bed = ok & ~ex.covered
        if (depth[bed] != F(ex.depth[bed])).any():
            fail(bed & (depth != F(ex.depth)), "background depth is not cam[2]")
        rel = np.abs(depth.astype(np.float64) / ex.depth - 1.0)
        if ex.exact:
            if (m & (depth != ex.depth.astype(F))).any() or (m & (ex.depth.astype(F).astype(np.float64) != ex.depth)).any():
                fail(m & (depth != ex.depth.astype(F)), "depth bits differ in an exact state")
        elif (m & (rel > ex.depth_bound)).any():
            fail(m & (rel > ex.depth_bound), "depth outside its bound (max %.3e of bound)" % float((rel[m] / ex.depth_bound[m]).max()))
        if m.any():
            stats["depth_rel"] = max(stats.get("depth_rel", 0.0), float(rel[m].max()))
            if not ex.exact:
                stats["depth_vs_bound"] = max(stats.get("depth_vs_bound", 0.0), float((rel[m] / ex.depth_bound[m]).max()))
                stats["depth_bound_max"] = max(stats.get("depth_bound_max", 0.0), float(ex.depth_bound[m].max()))
    stats["ambiguous"] = stats.get("ambiguous", 0) + int(ex.ambiguous.sum())
    stats["pixels"] = stats.get("pixels", 0) + ex.W * ex.H
    stats["cloth"] = stats.get("cloth", 0) + int(m.sum())
    return stats
