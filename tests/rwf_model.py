"""fp64 model of the random weight factorization of csrc/rwf.hip / pinn_rwf_split, pinn_rwf_compose and pinn_rwf_grad
(TEST INFRASTRUCTURE; numpy, plus a torch module for the autograd runs).  The definition (include/nsfnet_pinn.h), for a
net of Linear layers l = 0..L with rows_l x cols_l weights:

    g_l,i   = fp32(exp((double) s_l,i))                                   rounded once, used everywhere
    theta   = [params with V_l where W_l stands | s], P + R entries      R = sum rows_l, layers / rows ascending
    split   V[i,j] = fp32(W[i,j] / g_i)                                   b copied
    compose W[i,j] = fp32(g_i V[i,j])                                     b copied
    grad    dV[i,j] = g_i G[i,j],  db = G_b,  ds_i = g_i sum_j V[i,j] G[i,j]

split and compose return what the device must store (fp32, one rounding); grad returns the exact fp64 values of the
formulas on the fp32 inputs, and beside them the row sums of |V G| that the tests' error bound of ds is made of."""
import numpy as np
import torch


def layer_shapes(n_out, n_hidden, hidden):
    widths = [2] + [hidden] * n_hidden + [n_out]
    return [(widths[i + 1], widths[i]) for i in range(len(widths) - 1)]


def num_params(n_out, n_hidden, hidden):
    return sum(r * c + r for r, c in layer_shapes(n_out, n_hidden, hidden))


def num_rows(n_out, n_hidden, hidden):
    return sum(r for r, _ in layer_shapes(n_out, n_hidden, hidden))


def layout(n_out, n_hidden, hidden):
    """[(weight offset, bias offset, rows, cols, offset of the layer's s in the block behind the P parameters)]"""
    out, off, srow = [], 0, 0
    for r, c in layer_shapes(n_out, n_hidden, hidden):
        out.append((off, off + r * c, r, c, srow))
        off += r * c + r
        srow += r
    return out


def g_of(s):
    """fp32(exp((double) s))"""
    return np.exp(np.asarray(s, dtype=np.float32).astype(np.float64)).astype(np.float32)


def draw(seed, mean, std, nets):
    """The scale factors of set_weight_factorization: nets = [(n_out, n_hidden, hidden), ...] in drawing order (the
    main net first); one fp32 vector per net, every value drawn on its own, layers ascending and rows ascending."""
    rng = np.random.Generator(np.random.Philox(key=seed))
    out = []
    for shape in nets:
        vals = [rng.normal(mean, std) for rows, _ in layer_shapes(*shape) for _ in range(rows)]
        out.append(np.asarray(vals, dtype=np.float64).astype(np.float32))
    return out


def split(params, s, shape):
    params, s = np.asarray(params, dtype=np.float32), np.asarray(s, dtype=np.float32)
    P = num_params(*shape)
    theta = np.concatenate([params, s]).astype(np.float32)
    g = g_of(s)
    for w, b, r, c, so in layout(*shape):
        theta[w:b] = (params[w:b].reshape(r, c) / g[so:so + r, None]).reshape(-1)      # fp32 / fp32: one rounding
    assert theta.size == P + s.size
    return theta


def compose(theta, shape):
    theta = np.asarray(theta, dtype=np.float32)
    P = num_params(*shape)
    params = theta[:P].copy()
    g = g_of(theta[P:])
    for w, b, r, c, so in layout(*shape):
        params[w:b] = (g[so:so + r, None] * theta[w:b].reshape(r, c)).reshape(-1)      # fp32 * fp32: one rounding
    return params


def grad(theta, G, shape, exact_g=False):
    """(d loss / d theta, row sums of |V G| scaled by g) in fp64 from the fp32 (or, exact_g, fp64) theta and effective
    gradient G.  exact_g: g = exp(s) in fp64 without the rounding to fp32, the function torch autograd differentiates."""
    dt = np.float64 if exact_g else np.float32
    theta, G = np.asarray(theta, dtype=dt).astype(np.float64), np.asarray(G, dtype=dt).astype(np.float64)
    P = num_params(*shape)
    g = np.exp(theta[P:]) if exact_g else g_of(theta[P:]).astype(np.float64)
    out = np.zeros(theta.size)
    out[:P] = G
    mag = np.zeros(theta.size - P)
    for w, b, r, c, so in layout(*shape):
        V, Gw = theta[w:b].reshape(r, c), G[w:b].reshape(r, c)
        out[w:b] = (g[so:so + r, None] * Gw).reshape(-1)
        out[P + so:P + so + r] = g[so:so + r] * np.sum(V * Gw, axis=1)
        mag[so:so + r] = g[so:so + r] * np.sum(np.abs(V * Gw), axis=1)
    return out, mag


def bars(model, mag, shape):
    """The derived error bars of a device gtheta against grad()'s (model, mag): 2^-22 |model| everywhere (one ulp of
    difference in g plus one rounding), plus 2^-40 g_i sum_j |V G| on ds (the fp64 row sum in another order)."""
    P = num_params(*shape)
    bar = 2.0 ** -22 * np.abs(model)
    bar[P:] += 2.0 ** -40 * mag
    return bar


class RwfNet(torch.nn.Module):
    """The tanh MLP of oracle/autograd_ref.RefFCNet with every Linear weight written as diag(exp(s)) V.  parameters()
    come in theta's order: V_0, b_0, ..., V_L, b_L, then s_0 ... s_L."""

    def __init__(self, theta, shape, dtype=torch.float64):
        super().__init__()
        theta = torch.as_tensor(np.asarray(theta), dtype=dtype)
        P = num_params(*shape)
        vb = []
        for w, b, r, c, so in layout(*shape):
            vb.append((torch.nn.Parameter(theta[w:b].reshape(r, c).clone()), torch.nn.Parameter(theta[b:b + r].clone())))
        # registration order = parameters() order: V and b interleaved first, the scale factors last
        self.vb = torch.nn.ParameterList([p for pair in vb for p in pair])
        self.s = torch.nn.ParameterList([torch.nn.Parameter(theta[P + so:P + so + r].clone())
                                         for _, _, r, _, so in layout(*shape)])

    def weights(self):
        return [(torch.exp(self.s[l])[:, None] * self.vb[2 * l], self.vb[2 * l + 1]) for l in range(len(self.s))]

    def forward(self, X):
        h = X
        layers = self.weights()
        for l, (W, b) in enumerate(layers):
            h = h @ W.t() + b
            if l < len(layers) - 1:
                h = torch.tanh(h)
        return h

    def theta(self):
        return torch.cat([p.detach().reshape(-1) for p in self.parameters()])

    def effective(self):
        """The flat effective parameters (state_dict order)."""
        return torch.cat([t.detach().reshape(-1) for W, b in self.weights() for t in (W, b)])
