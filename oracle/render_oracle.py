"""numpy restatement of the cloth rasteriser (gym_cloth_amd/csrc/cloth_render.hpp), float32, same operation order.

TEST INFRASTRUCTURE, NOT PRODUCT CODE (only tests/ import it). There is no renderer to pin the images to outside Blender. This
file is a transliteration of the kernel, expression by expression: projection, smooth normals in face-index order, the edge
functions with the top-left rule, perspective-correct depth, two-sided colours, nearest-fragment-wins with the
(depth key, colour) tie-break. It pins the kernels' BITS (tests/test_gpu_render.py, test_gpu_render_obs.py); a rule written wrongly
the same way on both sides passes it. The RULES are pinned by oracle/render_exact.py, which states them geometrically and computes
them exactly, and which this file must meet too (tests/test_render_exact_host.py). The scene parameters it is called with follow the reference's Blender script
(gym_cloth/blender/get_image_rep_279.py: camera :114-122, lens :273-276, colours :249-257, bed :172)."""
import numpy as np

F = np.float32


def _q8(v):
    v = np.minimum(np.maximum(v, F(0.0)), F(1.0))
    return (v * F(255.0) + F(0.5)).astype(np.uint32)          # truncation, as the (uint32_t) cast


def faces(n_side):
    """The triangle list of the cloth mesh, in the order and with the winding the reference exports to Blender
    (gym_cloth/envs/cloth_env.py:224-229): per grid cell pp = r*N + c the two triangles [pp, pp+N, pp+1], [pp+1, pp+N, pp+N+1];
    vertex i = particle i. render() below rasterises exactly this list (tests pin it to the reference's captured export)."""
    N = int(n_side)
    out = []
    for r in range(N - 1):
        for c in range(N - 1):
            pp = r * N + c
            out.append((pp, pp + N, pp + 1))
            out.append((pp + 1, pp + N, pp + N + 1))
    return out


def render(pos, n_side, width, height, cam_pos, world_to_cam, lens_mm, sensor_mm, front, back, background, light_dir, ambient,
           energy, swap=False):
    """pos [P, 3] (any float type; converted to float32 as the kernel does) -> (rgb uint8 [H, W, 3], depth float32 [H, W])."""
    N, P, W, H = int(n_side), int(n_side) ** 2, int(width), int(height)
    w = np.asarray(pos).astype(F)
    cam = np.asarray(cam_pos, dtype=F); R = np.asarray(world_to_cam, dtype=F).reshape(9)
    front = np.asarray(front, dtype=F); back = np.asarray(back, dtype=F); bg = np.asarray(background, dtype=F)
    light = np.asarray(light_dir, dtype=F); ambient = F(ambient); energy = F(energy)
    fx = (F(lens_mm) / F(sensor_mm)) * F(W); fy = fx
    cx = F(0.5) * F(W); cy = F(0.5) * F(H)
    X, Y, Z = w[:, 0] - cam[0], w[:, 1] - cam[1], w[:, 2] - cam[2]
    xc = R[0] * X + R[1] * Y + R[2] * Z
    yc = R[3] * X + R[4] * Y + R[5] * Z
    zc = R[6] * X + R[7] * Y + R[8] * Z
    d = -zc
    ds = np.where(d > F(1e-6), d, F(1e-6))
    vx = (fx * xc) / ds + cx
    vy = cy - (fy * yc) / ds
    tri = faces(N)
    # vertex normals: incident faces in the kernel's order
    nrm = np.zeros((P, 3), dtype=F)
    for i in range(P):
        r, c = divmod(i, N)
        n = np.zeros(3, dtype=F)
        for qr in (r - 1, r):
            for qc in (c - 1, c):
                if qr < 0 or qc < 0 or qr >= N - 1 or qc >= N - 1:
                    continue
                pp = qr * N + qc
                for f in (tri[2 * (qr * (N - 1) + qc)], tri[2 * (qr * (N - 1) + qc) + 1]):
                    if i not in f:
                        continue
                    a, b, cc = f
                    u = w[b] - w[a]; t = w[cc] - w[a]
                    n = n + np.array([u[1] * t[2] - u[2] * t[1], u[2] * t[0] - u[0] * t[2], u[0] * t[1] - u[1] * t[0]], dtype=F)
        nrm[i] = n
    nn = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.where(nn > 0, (nrm[:, 0] * light[0] + nrm[:, 1] * light[1] + nrm[:, 2] * light[2]) / nn, F(0.0)).astype(F)
    lam = np.abs(lam)
    vi = (ambient + energy * lam).astype(F)
    bed_d = cam[2]
    bgkey = np.uint64((int(_q8(bg[0])) << 16) | (int(_q8(bg[1])) << 8) | int(_q8(bg[2])))      # depth key 0: behind everything
    zb = np.full((H, W), bgkey, dtype=np.uint64)
    for t in range(2 * (N - 1) * (N - 1)):
        a, b, c = tri[t]
        x0, y0, x1, y1, x2, y2 = vx[a], vy[a], vx[b], vy[b], vx[c], vy[c]
        if not (d[a] > F(1e-6) and d[b] > F(1e-6) and d[c] > F(1e-6)):
            continue
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if not (area > 0) and not (area < 0):
            continue
        is_front = (area < 0) != bool(swap)
        col = front if is_front else back
        mnx, mxx = max(min(x0, x1, x2), F(-1.0)), min(max(x0, x1, x2), F(W))
        mny, mxy = max(min(y0, y1, y2), F(-1.0)), min(max(y0, y1, y2), F(H))
        ix0, ix1 = max(int(np.floor(mnx)), 0), min(int(np.floor(mxx)), W - 1)
        iy0, iy1 = max(int(np.floor(mny)), 0), min(int(np.floor(mxy)), H - 1)
        if ix1 < ix0 or iy1 < iy0:
            continue
        s = F(1.0) if area > 0 else F(-1.0)
        iw0, iw1, iw2 = F(1.0) / d[a], F(1.0) / d[b], F(1.0) / d[c]
        fxp = (np.arange(ix0, ix1 + 1, dtype=F) + F(0.5))[None, :]
        fyp = (np.arange(iy0, iy1 + 1, dtype=F) + F(0.5))[:, None]
        e0 = s * ((x2 - x1) * (fyp - y1) - (y2 - y1) * (fxp - x1))
        e1 = s * ((x0 - x2) * (fyp - y2) - (y0 - y2) * (fxp - x2))
        e2 = s * ((x1 - x0) * (fyp - y0) - (y1 - y0) * (fxp - x0))
        tl0 = (s * (y2 - y1) < 0) or (y2 == y1 and s * (x2 - x1) > 0)
        tl1 = (s * (y0 - y2) < 0) or (y0 == y2 and s * (x0 - x2) > 0)
        tl2 = (s * (y1 - y0) < 0) or (y1 == y0 and s * (x1 - x0) > 0)
        inside = ((e0 > 0) | ((e0 == 0) & tl0)) & ((e1 > 0) | ((e1 == 0) & tl1)) & ((e2 > 0) | ((e2 == 0) & tl2))
        if not inside.any():
            continue
        sa = s * area
        b0, b1, b2 = e0 / sa, e1 / sa, e2 / sa
        inv_d = (b0 * iw0 + b1 * iw1 + b2 * iw2).astype(F)
        inten = (b0 * vi[a] + b1 * vi[b] + b2 * vi[c]).astype(F)
        key = (inv_d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
              ((_q8(col[0] * inten).astype(np.uint64) << np.uint64(16)) | (_q8(col[1] * inten).astype(np.uint64) << np.uint64(8)) |
               _q8(col[2] * inten).astype(np.uint64))
        sub = zb[iy0:iy1 + 1, ix0:ix1 + 1]
        sub[...] = np.where(inside, np.maximum(sub, key), sub)
    rgb = np.stack([(zb >> np.uint64(16)) & np.uint64(0xFF), (zb >> np.uint64(8)) & np.uint64(0xFF), zb & np.uint64(0xFF)], axis=-1).astype(np.uint8)
    kd = (zb >> np.uint64(32)).astype(np.uint32)
    with np.errstate(divide="ignore"):
        depth = np.where(kd == 0, bed_d, F(1.0) / kd.view(F)).astype(F)
    return rgb, depth
