"""float64 restatement of ONE normalised conv unit's apply / backward passes and of the SE / dropout side passes, per op.

The whole-net oracles (gunet2d.py, lgnet2d.py) evaluate these formulas inside a network through autograd; the kernel-level tests
need them per op, with the statistics GIVEN (mean, rstd, scale = gamma rstd, shift = beta - mean scale are inputs of the C entry
points), so the backward is written out in closed form here.  tests/test_norm_paths_host.py checks this closed form against
torch autograd through tf_ops.batch_norm / instance_norm where the given statistics are the true ones.

  t = y scale + shift,  xhat = (y - mean) rstd
  u = t den m + s                      (no leaky guide;  s = guide . gw + gb, m = dropout mask 0 | 1 / keep, den = density gain)
  u = t den m + act(s)                 (leaky guide: act = leaky ReLU of slope alpha, or the post form (s > 0 ? ap : an) s + ps)
  z = relu(u)
  du = dz [u > 0],  dt = du den m,  dg = du act'(s)
  dy = scale (dt - mean_g(dt) - xhat mean_g(dt xhat))          (means over the statistics group; affine_only: dy = scale dt)
  dbeta = sum dt, dgamma = sum dt xhat, dgw_g = sum dg guide_g, dgb = sum dg, dden[n] = sum_p du m t
  post: the gradient of the gb block [bias, ap, an, ps] is [sum dg, 0, 0, sum du]
(GUNet.py:119-133,154-156,181-214; LGNet.py:30-55; base.py:153-165.)
"""
import numpy as np


def _grp(a, per_sample, c):
    """[Ns, C] statistics -> broadcastable against [N, HW, C]."""
    a = np.asarray(a, np.float64)
    return a.reshape(-1, 1, c) if per_sample else a.reshape(1, 1, c)


def unit(y, dz, mean, rstd, scale, shift, per_sample, den=None, guide=None, gw=None, gb=None, mask=None, leaky=0, alpha=0.2,
         affine_only=False, per_sample_guide=False):
    """y, dz, mask [N, HW, C]; statistics [Ns, C]; den [N, C]; guide [N, HW, G]; gw [Ng, G, C]; gb [Ng, C] or, leaky == 3,
    [Ng, 4, C] (Ng = N with per_sample_guide, else 1).  leaky: 0 none, 1 / 2 leaky ReLU of slope alpha, 3 post block.
    Returns a dict of float64 arrays; `terms` holds the summands of every sum output (for exactness checks)."""
    y = np.asarray(y, np.float64)
    dz = np.asarray(dz, np.float64)
    n, hw, c = y.shape
    mu, rs, sc, sh = (_grp(a, per_sample, c) for a in (mean, rstd, scale, shift))
    t = y * sc + sh
    xh = (y - mu) * rs
    dn = 1.0 if den is None else np.asarray(den, np.float64)[:, None, :]
    m = 1.0 if mask is None else np.asarray(mask, np.float64)
    u = t * dn * m
    slope = 1.0
    g_ch = 0 if guide is None else guide.shape[-1]
    if gb is not None:
        gbv = np.asarray(gb, np.float64)
        blk = gbv if leaky == 3 else gbv[:, None, :]                 # [Ng, 4, C] rows bias, ap, an, ps
        s = np.broadcast_to(blk[:, 0][:, None, :], (n, hw, c))
        if g_ch:
            gwv = np.asarray(gw, np.float64)
            gwv = gwv if gwv.shape[0] == n else np.broadcast_to(gwv, (n,) + gwv.shape[1:])
            s = s + np.einsum("npg,ngc->npc", np.asarray(guide, np.float64), gwv)
        if leaky == 3:
            ap, an, ps = (blk[:, k][:, None, :] for k in (1, 2, 3))
            slope = np.where(s > 0, ap, an) * np.ones_like(s)
            u = u + slope * s + ps
        elif leaky:
            slope = np.where(s > 0, 1.0, alpha)
            u = u + slope * s
        else:
            u = u + s
    z = np.maximum(u, 0.0)
    du = dz * (u > 0)
    dt = du * dn * m
    dg = du * slope
    ax = (1,) if per_sample else (0, 1)
    cnt = float(hw if per_sample else n * hw)
    k1 = dt.sum(ax, keepdims=True)
    k2 = (dt * xh).sum(ax, keepdims=True)
    out = {"z": z, "u": u, "du": du, "xhat": xh}
    if affine_only:
        out["dy"] = sc * dt
        out["dy_steps"] = [dt]
    else:
        k1s, k2s = k1 / cnt, k2 / cnt
        prod = xh * k2s
        inner = dt - k1s - prod
        out["dy"] = sc * inner
        out["dy_steps"] = [k1s, k2s, prod, dt - k1s, inner]          # every value a contraction of the kernel's expression may form
    terms = {"dbeta": dt, "dgamma": dt * xh}
    tot = (lambda a: a.sum(1)) if per_sample_guide else (lambda a: a.sum((0, 1))[None])
    if g_ch:
        terms["dgw"] = dg[:, :, None, :] * np.asarray(guide, np.float64)[:, :, :, None]       # [N, HW, G, C]
        out["dgw"] = tot(terms["dgw"])
    if gb is not None:
        terms["dgb"] = dg if (den is not None or leaky) else dt
        row0 = tot(terms["dgb"])
        if leaky == 3:
            terms["dps"] = du
            zero = np.zeros_like(row0)
            out["dgb"] = np.stack([row0, zero, zero, tot(du)], 1)
        else:
            out["dgb"] = row0
    if den is not None:
        terms["dden"] = du * m * t
        out["dden"] = terms["dden"].sum(1)
    out["dbeta"] = dt.sum((0, 1))
    out["dgamma"] = (dt * xh).sum((0, 1))
    out["k1"], out["k2"] = k1, k2
    out["terms"] = terms
    return out


def window_view(a, n, h, w):
    """[N, H W, C] -> [N, H/2, W/2, 4, C], window positions in scan order (0,0), (0,1), (1,0), (1,1)."""
    c = a.shape[-1]
    return a.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 4, c)


def window_unview(a, n, h, w):
    c = a.shape[-1]
    return a.reshape(n, h // 2, w // 2, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h * w, c)


def pool_route(z_stored, dskip, dp, n, h, w, rnd=None):
    """TF MaxPoolGrad on the STORED activation: dz = rnd(dskip + (first maximum of the window in scan order ? dp : 0)).
    z_stored, dskip [N, H W, C]; dp [N, H/2 W/2, C]; rnd rounds to the storage type (None: fp32 storage, exact inputs)."""
    win = window_view(np.asarray(z_stored, np.float64), n, h, w)
    first = np.zeros_like(win)
    np.put_along_axis(first, win.argmax(3)[:, :, :, None, :], 1.0, 3)              # argmax = the first maximal index
    c = win.shape[-1]
    routed = first * np.asarray(dp, np.float64).reshape(n, h // 2, w // 2, 1, c)
    dz = np.asarray(dskip, np.float64) + window_unview(routed, n, h, w)
    return dz if rnd is None else rnd(dz)


def pooled(z_stored, n, h, w):
    c = z_stored.shape[-1]
    return window_view(np.asarray(z_stored, np.float64), n, h, w).max(3).reshape(n, (h // 2) * (w // 2), c)


def se_add(y, dy, mean, rstd, scale, a_mat, k2, per_sample):
    """SE gate without dropout (GUNet.py:191-201): pooled[b][c] = mean_p t reaches y a second time; the norm backward being linear
    in dt, dy += scale (A[b][c] - xhat k2[g][c]) with A = gate gradient / HW - its group mean, k2 = group mean of that times xhat."""
    y = np.asarray(y, np.float64)
    c = y.shape[-1]
    mu, rs, sc, kk = (_grp(a, per_sample, c) for a in (mean, rstd, scale, k2))
    xh = (y - mu) * rs
    return np.asarray(dy, np.float64) + sc * (np.asarray(a_mat, np.float64)[:, None, :] - xh * kk)


def drop_pool(y, mean, rstd, mask, per_sample):
    """SE gate with dropout, forward: sums[0][b][c] = sum_p m xhat, sums[1][b][c] = sum_p m (the gate pools the dropped-out value)."""
    y = np.asarray(y, np.float64)
    c = y.shape[-1]
    mu, rs = _grp(mean, per_sample, c), _grp(rstd, per_sample, c)
    m = np.asarray(mask, np.float64)
    return np.stack([(m * ((y - mu) * rs)).sum(1), m.sum(1)]), {"mx": m * ((y - mu) * rs), "m": m}


def se_add_drop(y, dy, mean, rstd, scale, e_mat, k1, k2, mask, per_sample):
    """... and backward: dy += scale (m E[b][c] - k1[g][c] - xhat k2[g][c])."""
    y = np.asarray(y, np.float64)
    c = y.shape[-1]
    mu, rs, sc, k1v, k2v = (_grp(a, per_sample, c) for a in (mean, rstd, scale, k1, k2))
    xh = (y - mu) * rs
    return np.asarray(dy, np.float64) + sc * (np.asarray(mask, np.float64) * np.asarray(e_mat, np.float64)[:, None, :] - k1v - xh * k2v)
