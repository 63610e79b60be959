"""Host half of the L-BFGS optimizer: torch.optim.LBFGS.step(closure) semantics (torch 2.10,
torch/optim/lbfgs.py) over an abstract vector space, so that the same logic drives the device
(PinnEngine.lbfgs_step: HIP kernels of csrc/lbfgs.hip) and a numpy model in the tests.

Only scalars live here.  The space holds the parameters x, the current gradient g (with whatever
rides along with it, e.g. the engine's loss sums), the direction d and the history, and answers:

  evaluate()        f(x) and g(x); returns (loss, g'd, max|g|) as host floats (one readback)
  direction(t_prev) new d from g and the history (t_prev = 0: first iteration, history emptied,
                    d = -g; t_prev < 0: a zero step, the pair s = 0 is rejected); returns
                    (g'd, max|d|, sum|g|, max|g|)
  save_x()          x0 = x
  set_x(t)          x = x0 + t d
  keep()            a handle on a copy of the current g (what torch's g.clone() is)
  restore(h)        make the kept gradient h current again
"""
import math


class LbfgsState:
    """What torch keeps in optimizer.state between step() calls; the vectors (d, history, g_prev) are the space's."""

    def __init__(self):
        self.n_iter = 0          # global iteration count: 0 means the next iteration is a first one
        self.func_evals = 0
        self.t = None
        self.prev_loss = None


def cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds=None):
    """torch.optim.lbfgs._cubic_interpolate on host floats."""
    if bounds is not None:
        xmin_bound, xmax_bound = bounds
    else:
        xmin_bound, xmax_bound = (x1, x2) if x1 <= x2 else (x2, x1)
    d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2)
    d2_square = d1 ** 2 - g1 * g2
    if d2_square >= 0:
        d2 = math.sqrt(d2_square)
        if x1 <= x2:
            min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2))
        else:
            min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2))
        return min(max(min_pos, xmin_bound), xmax_bound)
    return (xmin_bound + xmax_bound) / 2.0


def strong_wolfe(space, t, f, g, gtd, d_norm, c1=1e-4, c2=0.9, tolerance_change=1e-9, max_ls=25):
    """torch.optim.lbfgs._strong_wolfe.  g: a (handle, max|g|) pair of the gradient at t = 0.  Every gradient that
    torch keeps is kept as such a pair; the one of the accepted step is returned (it is not always the last
    evaluation).  Returns (f, (handle, max|g|), t, evaluations)."""
    def obj(t):
        space.set_x(t)
        f_new, gtd_new, gmax = space.evaluate()
        return f_new, (space.keep(), gmax), gtd_new

    f_new, g_new, gtd_new = obj(t)
    ls_func_evals = 1
    t_prev, f_prev, g_prev, gtd_prev = 0, f, g, gtd
    done = False
    ls_iter = 0
    while ls_iter < max_ls:
        if f_new > (f + c1 * t * gtd) or (ls_iter > 1 and f_new >= f_prev):
            bracket, bracket_f, bracket_g, bracket_gtd = [t_prev, t], [f_prev, f_new], [g_prev, g_new], [gtd_prev, gtd_new]
            break
        if abs(gtd_new) <= -c2 * gtd:
            bracket, bracket_f, bracket_g = [t], [f_new], [g_new]
            done = True
            break
        if gtd_new >= 0:
            bracket, bracket_f, bracket_g, bracket_gtd = [t_prev, t], [f_prev, f_new], [g_prev, g_new], [gtd_prev, gtd_new]
            break
        min_step = t + 0.01 * (t - t_prev)
        max_step = t * 10
        tmp = t
        t = cubic_interpolate(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, bounds=(min_step, max_step))
        t_prev, f_prev, g_prev, gtd_prev = tmp, f_new, g_new, gtd_new
        f_new, g_new, gtd_new = obj(t)
        ls_func_evals += 1
        ls_iter += 1

    if ls_iter == max_ls:
        bracket, bracket_f, bracket_g = [0, t], [f, f_new], [g, g_new]

    insuf_progress = False
    low_pos, high_pos = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0)
    while not done and ls_iter < max_ls:
        if abs(bracket[1] - bracket[0]) * d_norm < tolerance_change:
            break
        t = cubic_interpolate(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1])
        eps = 0.1 * (max(bracket) - min(bracket))
        if min(max(bracket) - t, t - min(bracket)) < eps:
            if insuf_progress or t >= max(bracket) or t <= min(bracket):
                if abs(t - max(bracket)) < abs(t - min(bracket)):
                    t = max(bracket) - eps
                else:
                    t = min(bracket) + eps
                insuf_progress = False
            else:
                insuf_progress = True
        else:
            insuf_progress = False
        f_new, g_new, gtd_new = obj(t)
        ls_func_evals += 1
        ls_iter += 1
        if f_new > (f + c1 * t * gtd) or f_new >= bracket_f[low_pos]:
            bracket[high_pos], bracket_f[high_pos], bracket_g[high_pos], bracket_gtd[high_pos] = t, f_new, g_new, gtd_new
            low_pos, high_pos = (0, 1) if bracket_f[0] <= bracket_f[1] else (1, 0)
        else:
            if abs(gtd_new) <= -c2 * gtd:
                done = True
            elif gtd_new * (bracket[high_pos] - bracket[low_pos]) >= 0:
                bracket[high_pos] = bracket[low_pos]
                bracket_f[high_pos] = bracket_f[low_pos]
                bracket_g[high_pos] = bracket_g[low_pos]
                bracket_gtd[high_pos] = bracket_gtd[low_pos]
            bracket[low_pos], bracket_f[low_pos], bracket_g[low_pos], bracket_gtd[low_pos] = t, f_new, g_new, gtd_new

    return bracket_f[low_pos], bracket_g[low_pos], bracket[low_pos], ls_func_evals


def check_knobs(lr, max_iter, max_eval, history_size, line_search_fn):
    if line_search_fn not in (None, "strong_wolfe"):
        raise ValueError("line_search_fn must be None or 'strong_wolfe' (got %r)" % (line_search_fn,))
    if not (lr > 0) or not math.isfinite(lr):
        raise ValueError("lr must be finite and > 0")
    if int(max_iter) < 1 or int(history_size) < 1:
        raise ValueError("max_iter and history_size must be >= 1")
    return int(max_iter * 5 // 4) if max_eval is None else int(max_eval)


def step(space, state, lr=1.0, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9,
         line_search_fn=None):
    """One torch.optim.LBFGS.step(closure).  Returns (loss at entry, info) with info = dict(evals, iters, reason):
    reason in 'max_iter', 'max_eval', 'tolerance_grad' (max|g| at or below it, also at entry), 'tolerance_change'
    (max|t d| at or below it), 'loss_change' (|f - f_prev| below tolerance_change), 'gtd' (directional derivative
    above -tolerance_change)."""
    max_eval = check_knobs(lr, max_iter, max_eval, 1, line_search_fn)
    orig_loss, _, gmax = space.evaluate()
    loss = orig_loss
    current_evals = 1
    state.func_evals += 1
    if gmax <= tolerance_grad:
        return orig_loss, dict(evals=current_evals, iters=0, reason="tolerance_grad")
    t = state.t
    n_iter = 0
    reason = "max_iter"
    while n_iter < max_iter:
        n_iter += 1
        state.n_iter += 1
        first = state.n_iter == 1
        # t_prev: 0 = first iteration; a zero step of a later one (the line search accepted t = 0) is passed as -1
        gtd, d_norm, g1, gmax = space.direction(0.0 if first else (t if t > 0 else -1.0))
        state.prev_loss = prev_loss = loss
        t = min(1.0, 1.0 / g1) * lr if first else lr
        if gtd > -tolerance_change:
            reason = "gtd"
            break
        ls_func_evals = 0
        opt_cond = False
        if line_search_fn is not None:
            space.save_x()
            h0 = (space.keep(), gmax)
            # (torch passes no tolerance_change here: the zoom phase's bracket exit keeps its default 1e-9)
            loss, (h, gmax), t, ls_func_evals = strong_wolfe(space, t, loss, h0, gtd, d_norm,
                                                            max_ls=max_eval - current_evals)
            space.set_x(t)
            space.restore(h)
            opt_cond = gmax <= tolerance_grad
        else:
            space.save_x()
            space.set_x(t)
            if n_iter != max_iter:
                loss, _, gmax = space.evaluate()
                opt_cond = gmax <= tolerance_grad
                ls_func_evals = 1
        current_evals += ls_func_evals
        state.func_evals += ls_func_evals
        if n_iter == max_iter:
            reason = "max_iter"
            break
        if current_evals >= max_eval:
            reason = "max_eval"
            break
        if opt_cond:
            reason = "tolerance_grad"
            break
        if abs(t) * d_norm <= tolerance_change:      # max|t d| (rounding is monotone: the same number)
            reason = "tolerance_change"
            break
        if abs(loss - prev_loss) < tolerance_change:
            reason = "loss_change"
            break
    state.t = t
    return orig_loss, dict(evals=current_evals, iters=n_iter, reason=reason)
