"""Float64 reference of lnerf_render_maps_vjp: the vector-Jacobian product of the render maps
(colour, depth, opacity, per-sample weights, rgba) with the caller's adjoints, back to dW, db, dX
and d_dists.

The forward is the MLP of oracle/nerf_np.py (nerf.py:134-167: ReLU hidden layers, sigmoid rgb,
ReLU sigma) followed by render_maps_ref.composite64 (the reference's inclusive transmittance,
T_0 = 1). The reverse seeds each sample with

    dw_j      = rgb_j . dC + t_j dD + dO + dWt_j
    drgb_j    = w_j dC + dRGBA_j[0..2]
    dsigma_j += dRGBA_j[3]        (before the ReLU gate sigma > 0: rgba's sigma is the post-ReLU value)

and then runs nerf_np.nerf_forward_backward's own reverse: dal = T dw, the suffix recurrence
G_j = a_j + c_{j+1} G_{j+1}, dc, the alpha reverse, the head and the MLP chain. `masks` are the hidden
ReLU decisions to use instead of z > 0 in both passes, as nerf_np.nerf_forward_backward(masks=) takes
another implementation's. tests/test_render_vjp_ref.py checks this file against nerf_np and against
central differences before it judges the GPU.
"""
import numpy as np

from render_maps_ref import composite64

ADJOINTS = ("color", "depth", "opacity", "weights", "rgba")


def forward64(X, ws, bs, dists, S, t=None, masks=None):
    """The float64 forward: dict with the maps (color (N, 3), depth (N) or None, opacity (N), weights
    (N, S), rgba (N S, 4)) and the intermediates the reverse needs."""
    X = np.asarray(X, np.float64)
    L = len(ws)
    A, Z = [X], []
    for l in range(L):
        z = A[-1] @ np.asarray(ws[l], np.float64) + np.asarray(bs[l], np.float64)[None, :]
        Z.append(z)
        if l < L - 1:
            m = (z > 0) if masks is None else np.asarray(masks[l], bool)
            A.append(np.where(m, z, 0.0))
    zl = Z[-1]
    N = X.shape[0] // S
    rgb = (1.0 / (1.0 + np.exp(-zl[:, :3]))).reshape(N, S, 3)
    sigma = np.where(zl[:, 3] > 0, zl[:, 3], 0.0).reshape(N, S)
    dl = np.asarray(dists, np.float64).reshape(N, S)
    maps = composite64(rgb, sigma, dl, None if t is None else np.asarray(t, np.float64).reshape(N, S))
    maps["rgba"] = np.concatenate([rgb, sigma[:, :, None]], axis=2).reshape(N * S, 4)
    maps.update(A=A, Z=Z, rgb=rgb, sigma=sigma, dl=dl)
    return maps


def pairing(maps, adj):
    """sum(C dC) + sum(D dD) + sum(O dO) + sum(w dWt) + sum(rgba dRGBA): the scalar whose gradient the
    VJP is."""
    s = 0.0
    for k in ADJOINTS:
        if adj.get(k) is not None:
            s += float((np.asarray(maps[k], np.float64) * np.asarray(adj[k], np.float64).reshape(maps[k].shape)).sum())
    return s


def render_vjp64(X, ws, bs, dists, S, adj, t=None, masks=None):
    """adj: dict of ADJOINTS -> arrays (color (N, 3), depth (N), opacity (N), weights (N, S), rgba
    (N S, 4)); a missing / None entry contributes nothing. t (N, S): the sample depths (needed with a
    depth adjoint). Returns dict(dW, db per layer, dX, d_dists (N, S), and the forward's maps)."""
    f = forward64(X, ws, bs, dists, S, t, masks)
    rgb, sg, dl, A, Z = f["rgb"], f["sigma"], f["dl"], f["A"], f["Z"]
    N, L = rgb.shape[0], len(ws)
    get = lambda k, shape: None if adj.get(k) is None else np.asarray(adj[k], np.float64).reshape(shape)
    dC, dD, dO = get("color", (N, 3)), get("depth", (N,)), get("opacity", (N,))
    dWt, dR = get("weights", (N, S)), get("rgba", (N, S, 4))
    e = np.exp(-sg * dl)
    alpha = 1.0 - e
    c = (1.0 - alpha) + 1e-10
    P = np.cumprod(c, axis=1)
    T = P.copy()
    T[:, 0] = 1.0
    w = alpha * T
    # the seeds
    gw = np.zeros((N, S))
    grgb = np.zeros((N, S, 3))
    if dC is not None:
        gw += (dC[:, None, :] * rgb).sum(2)
        grgb += w[:, :, None] * dC[:, None, :]
    if dD is not None:
        gw += np.asarray(t, np.float64).reshape(N, S) * dD[:, None]
    if dO is not None:
        gw += dO[:, None]
    if dWt is not None:
        gw += dWt
    if dR is not None:
        grgb += dR[:, :, :3]
    # nerf_np.nerf_forward_backward's reverse from here
    dP = alpha * gw
    dP[:, 0] = 0.0
    dc = np.zeros_like(c)
    for j in range(S - 1, 0, -1):
        dP[:, j - 1] += dP[:, j] * c[:, j]
        dc[:, j] += dP[:, j] * P[:, j - 1]
    dc[:, 0] += dP[:, 0]
    galpha = T * gw - dc
    gsigma = galpha * e * dl
    gdist = galpha * e * sg
    if dR is not None:
        gsigma = gsigma + dR[:, :, 3]
    zl = Z[-1]
    dz = np.zeros_like(zl)
    s3 = rgb.reshape(-1, 3)
    dz[:, :3] = grgb.reshape(-1, 3) * s3 * (1.0 - s3)
    dz[:, 3] = np.where(zl[:, 3] > 0, gsigma.reshape(-1), 0.0)
    dW, db = [None] * L, [None] * L
    g, dX = dz, None
    for l in range(L - 1, -1, -1):
        dW[l] = A[l].T @ g
        db[l] = g.sum(0)
        ga = g @ np.asarray(ws[l], np.float64).T
        if l > 0:
            m = (Z[l - 1] > 0) if masks is None else np.asarray(masks[l - 1], bool)
            g = np.where(m, ga, 0.0)
        else:
            dX = ga
    return dict(dW=dW, db=db, dX=dX, d_dists=gdist, maps=f)


def random_adjoints(N, S, seed, kinds=ADJOINTS):
    """Unit-scale random adjoints (float32) of the named kinds."""
    rng = np.random.RandomState(seed)
    shapes = dict(color=(N, 3), depth=(N,), opacity=(N,), weights=(N, S), rgba=(N * S, 4))
    full = {k: rng.randn(*shapes[k]).astype(np.float32) for k in ADJOINTS}   # one stream whatever `kinds`
    return {k: full[k] for k in kinds}
