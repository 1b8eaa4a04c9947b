"""The small fully-connected network as plain numpy (numpy only, nothing of the package): how a list of (W, b) layers is laid out for the
library (pack_mlp / unpack_mlp / pack_population, which batch.py, envs.py, policies.py and trainers.py share), and the ONE float64 pass
-- mlp_float64, mlp_forward, mlp_backward -- that every numpy reference of the network rests on (references.py, MLPPolicy.reference)."""
import numpy as np

MLP_MAX_LAYERS, MLP_MAX_WIDTH = 4, 256


def pack_mlp(layers, n_in=None, n_out=4):
    """[(W, b), ...] -> (widths int32[L + 1], blob float32): for every layer W [out, in] row-major (torch.nn.Linear.weight's layout),
    then b [out] -- what clothhip_set_policy_mlp takes. ValueError for anything the library would refuse: no or more than four layers,
    a W that is not 2-d or a b that is not [out], widths that do not chain, an input width other than n_in (when given), a last width
    other than 4 (n_out: 1 for a value network, clothhip_set_value_mlp), a hidden width outside [1, 256], non-finite values."""
    layers = list(layers)
    if not 1 <= len(layers) <= MLP_MAX_LAYERS:
        raise ValueError("an MLP policy has 1 to %d weight layers (got %d)" % (MLP_MAX_LAYERS, len(layers)))
    widths, parts = [], []
    for l, wb in enumerate(layers):
        if len(wb) != 2:
            raise ValueError("layer %d must be a (W, b) pair" % l)
        W, b = np.asarray(wb[0], dtype=np.float32), np.asarray(wb[1], dtype=np.float32)
        if W.ndim != 2 or W.shape[0] < 1 or W.shape[1] < 1:
            raise ValueError("layer %d: W must be a non-empty [out, in] matrix (got shape %r)" % (l, W.shape))
        if b.shape != (W.shape[0],):
            raise ValueError("layer %d: b must have shape (%d,) (got %r)" % (l, W.shape[0], b.shape))
        if l and W.shape[1] != widths[-1]:
            raise ValueError("layer %d takes %d inputs, layer %d gives %d" % (l, W.shape[1], l - 1, widths[-1]))
        if not (np.isfinite(W).all() and np.isfinite(b).all()):
            raise ValueError("layer %d holds non-finite values" % l)
        if not l:
            widths.append(int(W.shape[1]))
        widths.append(int(W.shape[0]))
        parts += [np.ascontiguousarray(W).reshape(-1), b]
    if n_in is not None and widths[0] != int(n_in):
        raise ValueError("the network's input width is %d, the '1d' observation has %d values" % (widths[0], int(n_in)))
    if widths[-1] != int(n_out):
        raise ValueError("the network's output width is %d, %s" % (widths[-1], "an action has 4 values" if int(n_out) == 4 else "this network has %d" % int(n_out)))
    for l in range(1, len(widths) - 1):
        if not 1 <= widths[l] <= MLP_MAX_WIDTH:
            raise ValueError("hidden width %d (layer %d) outside [1, %d]" % (widths[l], l, MLP_MAX_WIDTH))
    return np.asarray(widths, dtype=np.int32), np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


def unpack_mlp(widths, blob):
    """The inverse of pack_mlp: [(W, b), ...] float32 copies out of one blob."""
    layers, o = [], 0
    for l in range(len(widths) - 1):
        n_in, n_out = int(widths[l]), int(widths[l + 1])
        W = np.array(blob[o:o + n_out * n_in], dtype=np.float32).reshape(n_out, n_in); o += n_out * n_in
        b = np.array(blob[o:o + n_out], dtype=np.float32); o += n_out
        layers.append((W, b))
    if o != len(blob):
        raise ValueError("the blob holds %d values, these widths %d" % (len(blob), o))
    return layers


def pack_population(members, n_in=None):
    """[network, ...] (each a list of (W, b) layers, all of ONE shape) -> (widths int32[L + 1], float32 [G, n_params]): what
    clothhip_set_policy_population takes. ValueError for what pack_mlp refuses, and for networks of different shapes."""
    members = list(members)
    if not members:
        raise ValueError("a population has at least one network")
    widths, rows = None, []
    for g, layers in enumerate(members):
        w, blob = pack_mlp(layers, n_in=n_in)
        if widths is not None and not np.array_equal(w, widths):
            raise ValueError("network %d has widths %r, network 0 has %r: a population has one shape" % (g, w.tolist(), widths.tolist()))
        widths = w
        rows.append(blob)
    return widths, np.ascontiguousarray(np.stack(rows), dtype=np.float32)


def population_stride(n_params):
    """Floats between two rows of a population on the device: n_params rounded up to 64, so that every row is 256-byte aligned."""
    return (int(n_params) + 63) // 64 * 64


def mlp_float64(layers):
    """[(W, b), ...] -> (Ws, bs) in float64, rounded to float32 first: the weights as the device stores them."""
    Ws = [np.asarray(W, dtype=np.float32).astype(np.float64) for W, _ in layers]
    bs = [np.asarray(b, dtype=np.float32).astype(np.float64) for _, b in layers]
    return Ws, bs


def mlp_forward(Ws, bs, x):
    """The activations hs = [x, h_1, ..., y] of the rows x [B, in], float64: ReLU after every layer but the last."""
    L, hs = len(Ws), [x]
    for l in range(L):
        z = hs[-1] @ Ws[l].T + bs[l]
        hs.append(np.maximum(z, 0.0) if l + 1 < L else z)
    return hs


def mlp_backward(Ws, hs, g):
    """[(dW, db), ...] in the layers' shapes from g = dL/dy [B, out] and the forward's hs; ReLU' = 1 where the activation is > 0, else 0."""
    grads = [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        grads[l] = (g.T @ hs[l], g.sum(axis=0))
        if l:
            g = (g @ Ws[l]) * (hs[l] > 0.0)
    return grads
