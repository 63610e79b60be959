"""fp64 numpy model of the L-BFGS direction kernels (csrc/lbfgs.hip) and an fp64 two-loop recursion
(TEST INFRASTRUCTURE).  The model keeps the kernels' bookkeeping: history_size + 1 physical slots, a
staging slot for the candidate pair, R and Y'Y indexed by physical slot, the compact-form solve."""
import numpy as np
import torch


class LbfgsModel:
    def __init__(self, n, m):
        self.n, self.m = int(n), int(m)
        self.S = np.zeros((m + 1, n))
        self.Y = np.zeros((m + 1, n))
        self.R = np.zeros((m + 1, m + 1))
        self.YY = np.zeros((m + 1, m + 1))
        self.g_prev = np.zeros(n)
        self.d = np.zeros(n)
        self.reset()

    def reset(self):
        self.order, self.staging, self.gamma, self.accepted, self.ys = [], 0, 1.0, -1, 0.0

    def pairs(self):
        """Live (s, y) pairs, oldest first (copies)."""
        return [(self.S[j].copy(), self.Y[j].copy()) for j in self.order]

    def direction(self, g, t_prev):
        g = np.asarray(g, dtype=np.float64)
        if t_prev == 0:
            self.reset()
            self.d = -g
        else:
            st = self.staging
            self.S[st] = max(t_prev, 0.0) * self.d          # t_prev < 0: a zero step
            self.Y[st] = g - self.g_prev
            s, y = self.S[st], self.Y[st]
            ys, yy = float(y @ s), float(y @ y)
            self.ys = ys
            self.accepted = 1 if ys > 1e-10 else 0
            if self.accepted:
                dropped = None
                if len(self.order) == self.m:
                    dropped = self.order.pop(0)
                for j in self.order:
                    self.R[j, st] = self.S[j] @ y
                    self.YY[j, st] = self.YY[st, j] = self.Y[j] @ y
                self.R[st, st], self.YY[st, st] = ys, yy
                self.order.append(st)
                self.staging = dropped if dropped is not None else len(self.order)
                self.gamma = ys / yy
            self.d = self.compact(g)
        self.g_prev = g.copy()
        return self.stats(g)

    def compact(self, g):
        o, gam = self.order, self.gamma
        if not o:
            return -gam * g
        R = np.triu(self.R[np.ix_(o, o)])
        YY = self.YY[np.ix_(o, o)]
        a = np.array([self.S[j] @ g for j in o])          # row by row: no copy of the history (large n)
        b = np.array([self.Y[j] @ g for j in o])
        u = np.linalg.solve(R, a)
        p = np.linalg.solve(R.T, (np.diag(np.diag(R)) + gam * YY) @ u - gam * b)
        d = -gam * g
        for k, j in enumerate(o):
            d -= p[k] * self.S[j]
            d += (gam * u[k]) * self.Y[j]
        return d

    def stats(self, g, d=None):
        d = self.d if d is None else d
        return np.array([g @ d, np.abs(d).max(), np.abs(g).sum(), np.abs(g).max(),
                         self.accepted, len(self.order), self.gamma, self.ys])


def two_loop(g, pairs, gamma):
    """torch.optim.LBFGS's direction (fp64): pairs = [(s, y)] oldest first, H0 = gamma I."""
    q = -np.asarray(g, dtype=np.float64)
    al = [0.0] * len(pairs)
    for i in range(len(pairs) - 1, -1, -1):
        s, y = pairs[i]
        al[i] = (s @ q) / (y @ s)
        q = q - al[i] * y
    r = q * gamma
    for i, (s, y) in enumerate(pairs):
        be = (y @ r) / (y @ s)
        r = r + s * (al[i] - be)
    return r


class ModelHistory:
    """Drop-in for engine.LbfgsHistory on CPU tensors (the gloo tests swap it in, as tests/fakes.py does for plans)."""

    def __init__(self, n, history_size, device):
        self.n, self.history_size = int(n), int(history_size)
        self.model = LbfgsModel(n, history_size)
        self.d = torch.zeros(self.n, dtype=torch.float32)
        self.x0 = torch.zeros(self.n, dtype=torch.float32)

    def reset(self):
        self.model.reset()

    def direction(self, g, t_prev):
        self.model.d = self.d.double().numpy()
        r = self.model.direction(g.double().numpy(), float(t_prev))
        self.d.copy_(torch.tensor(self.model.d, dtype=torch.float32))
        self.model.d = self.d.double().numpy()
        return torch.tensor(r, dtype=torch.float64)

    def probe(self, g):
        return torch.tensor(self.model.stats(g.double().numpy(), self.d.double().numpy()), dtype=torch.float64)


class NumpySpace:
    """lbfgs.step's vector space over an fp64 objective f(x) -> (loss, grad) and the model."""

    def __init__(self, fun, x, m):
        self.fun, self.x = fun, np.array(x, dtype=np.float64)
        self.h = LbfgsModel(self.x.size, m)
        self.g = None
        self.losses = []

    def evaluate(self):
        f, self.g = self.fun(self.x)
        self.losses.append(float(f))
        return float(f), float(self.g @ self.h.d), float(np.abs(self.g).max())

    def direction(self, t_prev):
        r = self.h.direction(self.g, t_prev)
        return float(r[0]), float(r[1]), float(r[2]), float(r[3])

    def save_x(self):
        self.x0 = self.x.copy()

    def set_x(self, t):
        self.x = self.x0 + t * self.h.d

    def keep(self):
        return self.g.copy()

    def restore(self, h):
        self.g = h.copy()
