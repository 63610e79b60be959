"""GPU tests of the training-state snapshots: the pack / unpack kernel against the numpy model
of tests/state_model.py (payload bytes, zero padding, digests), and the engine: K updates, save, a NEW engine with
other weights, load, K more against 2K in one go - every state tensor and the loss terms bit for bit, per training
option -, a load under captured graphs, and the non-blocking snapshot.  All comparisons are exact."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import state_model as sm  # noqa: E402
from oracle import autograd_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = 7
LR = 1e-3


# ---------------------------------------------------------------- the kernel against the model
def _segments(count, seed, big):
    """`count` host arrays (uint8 views of random words) with the sizes where the kernel changes path: empty, below and
    at one 16-byte access, tails, one chunk (16 KiB) -4 / exact / +4, several chunks, and - big - 32 MiB of ones, more
    than the grid's 1024 x 16 KiB, so the chunk loop repeats and B wraps 2^64."""
    rng = np.random.RandomState(seed)
    sizes = [0, 4, 12, 16, 20, 16384 - 4, 16384, 16384 + 4, 0, 3 * 16384 + 40, 256, 260]
    sizes += [int(4 * rng.randint(0, 3000)) for _ in range(count - len(sizes) - (1 if big else 0))]
    arrays = [rng.randint(0, 256, s).astype(np.uint8) for s in sizes]
    if big:
        arrays.insert(5, np.full(32 << 20, 0xFF, dtype=np.uint8))
    return arrays


def _device(arrays, misaligned):
    """Device tensors of the arrays; the ones listed in `misaligned` are views one float into their allocation (4-byte
    aligned only)."""
    out = []
    for k, a in enumerate(arrays):
        if k in misaligned:
            buf = torch.zeros(a.size + 4, dtype=torch.uint8, device=DEV)
            buf[4:].copy_(torch.from_numpy(a))
            out.append(buf[4:])
            assert a.size == 0 or out[-1].data_ptr() % 16 == 4
        else:
            out.append(torch.from_numpy(a).to(DEV))
    return out


def _digest_rows(t):
    return [tuple(int(v) for v in row) for row in t.cpu().numpy().view(np.uint64)]


@pytest.mark.parametrize("count,big", [(64, True), (150, False)])
def test_pack_and_unpack_match_the_model(count, big):
    """64 segments in one launch, and 150 in three."""
    from nsfnet_amd import engine as eng
    from nsfnet_amd import state_file
    arrays = _segments(count, count, big)
    stored = [k != 3 and k != 20 for k in range(count)]                 # two digest-only segments
    mis = {7, 9, 13}
    want, offsets, digests = sm.pack(arrays, stored)
    offs, total = state_file.layout([a.size if s else 0 for a, s in zip(arrays, stored)])
    assert total == len(want) and [o if s else -1 for o, s in zip(offs, stored)] == offsets
    src = _device(arrays, mis)
    staging = torch.full((total,), 0xAB, dtype=torch.uint8, device=DEV)     # the padding must be written, not assumed
    dig = torch.zeros(count, 2, dtype=torch.int64, device=DEV)
    scratch = eng.state_scratch(DEV)
    eng.state_pack(src, offsets, staging, dig, scratch)
    torch.cuda.synchronize()
    got = staging.cpu().numpy()
    used = np.zeros(total, dtype=bool)
    for a, o in zip(arrays, offsets):
        if o >= 0:
            used[o:sm.align256(o + a.size)] = True
    np.testing.assert_array_equal(got[used], np.frombuffer(want, dtype=np.uint8)[used])
    assert _digest_rows(dig) == digests
    assert float(scratch[0].item()) == 0.0                                  # the ticket is 0 again
    # the reverse scatter into poisoned buffers, the misaligned ones included; digest-only ones are read, not written
    dst = _device([np.full(a.size, 0x5A, dtype=np.uint8) for a in arrays], mis)
    for k, s in enumerate(stored):
        if not s:
            dst[k].copy_(src[k])
    staging2 = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).to(DEV)
    dig.zero_()
    eng.state_unpack(staging2, offsets, dst, dig, scratch)
    torch.cuda.synchronize()
    for k, (a, d) in enumerate(zip(arrays, dst)):
        np.testing.assert_array_equal(d.cpu().numpy(), a, err_msg="segment %d" % k)
    assert _digest_rows(dig) == digests


def test_bad_segments_are_refused_before_a_launch():
    from nsfnet_amd import _lib
    from nsfnet_amd import engine as eng
    scratch, dig = eng.state_scratch(DEV), torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    a = torch.zeros(64, dtype=torch.uint8, device=DEV)
    staging = torch.zeros(256, dtype=torch.uint8, device=DEV)
    for srcs, offsets, what in (([a[:6]], [0], "multiple of 4"), ([a, a], [0, 0], "overlaps"), ([a], [128], "multiple of 256"),
                                ([a, a], [0, 256], "runs past"), ([a[1:5]], [0], "4-byte aligned")):
        with pytest.raises(_lib.PinnLibraryError, match=what):
            eng.state_pack(srcs, offsets, staging, dig, scratch)


# ---------------------------------------------------------------- the engine
def _points(n, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)


def _boundary():
    return tuple(a.reshape(-1)[::16].astype(np.float32) for a in ar.cavity_boundary())


def _engine(seed, n_hidden, hidden, n, ev=None, precision="fp32", before=None, after=None, weights=False, sup=False):
    """An engine with its data attached: `before` runs ahead of every point set, `after` behind them."""
    from nsfnet_amd import engine as eng
    kw = {} if ev is None else dict(flavour="ev", n_hidden_e=ev[0], hidden_e=ev[1], alpha_evm=0.03)
    e = eng.PinnEngine(DEV, n_hidden, hidden, 400.0, alpha_b=10.0, alpha_e=1.0, alpha_s=2.0 if sup else 0.0,
                       precision=precision, **kw)
    rng = np.random.RandomState(seed)
    e.net.set_flat(torch.tensor(rng.randn(e.P) * 0.2, dtype=torch.float32))
    if ev is not None:
        e.net_e.set_flat(torch.tensor(rng.randn(e.P1) * 0.2, dtype=torch.float32))
    if before is not None:
        before(e)
    x, y = _points(n, 1)
    e.set_collocation(x, y, (0.5 + x).astype(np.float32) if weights else None)
    e.set_boundary(*_boundary())
    if sup:
        xs, ys = _points(130, 2)
        p = (xs * ys).astype(np.float32)
        p[::3] = np.nan
        e.set_supervised(xs, ys, np.sin(xs), np.cos(ys), p)
    if after is not None:
        after(e)
    return e


def _state(e, loss=True):
    torch.cuda.synchronize()
    out = {name: t.detach().cpu().numpy().copy() for name, t, stored in e._state_segments() if stored}
    out["params"] = e.net.params.cpu().numpy().copy()
    out["prep"] = e.net.prep.cpu().numpy().copy()
    out["host"] = e._state_host()
    if loss:
        out["loss"] = {k: np.asarray(torch.as_tensor(v).cpu()) for k, v in e.loss_terms().items()}
    return out


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    assert a["host"] == b["host"]
    for k in a:
        if k == "loss":
            for name in a[k]:
                np.testing.assert_array_equal(a[k][name], b[k][name], err_msg=name)
        elif k != "host":
            np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)


def _continuation(tmp_path, make, advance, k=K):
    """2k updates in one go against k, save, a NEW engine with other initial weights, load, k more."""
    whole = make(5)
    for i in range(2 * k):
        advance(whole, i)
    want = _state(whole)
    first = make(5)
    for i in range(k):
        advance(first, i)
    path = str(tmp_path / "state.bin")
    first.save_training_state(path, extra=dict(next=k))
    del first
    second = make(77)
    assert second.load_training_state(path) == dict(extra=dict(next=k), changed=[])
    for i in range(k, 2 * k):
        advance(second, i)
    _assert_same(want, _state(second))
    return whole, second


def _step(e, i):
    e.step(LR)


def test_plain_fp32_continues(tmp_path):
    whole, second = _continuation(tmp_path, lambda seed: _engine(seed, 4, 50, 1000), _step)
    assert second.net.adam_t == 2 * K == int(second.net.adam_t_dev[0].item())


def test_ev_with_schedule_rwf_attention_balancing_validation_continues(tmp_path):
    from nsfnet_amd import schedule
    xv, yv = _points(300, 3)

    def after(e):
        e.set_weight_factorization(mean=0.5, std=0.1, seed=3)
        e.set_lr_schedule(schedule.LrSchedule("cosine", t_max=40, warmup_epochs=5))
        e.set_grad_clipping(0.5)
        e.set_residual_attention(eta=0.05, gamma=0.9)
        e.set_loss_balancing(every=3, beta=0.2)
        e.set_validation(xv, yv, np.sin(3 * xv) * yv, np.cos(2 * yv) * xv, 0.2 + xv * yv, every=5, keep_best=True, history=2)

    def advance(e, i):
        if i in (3, 4, 9):
            e.e_trainable = not e.e_trainable
            if e.e_trainable:
                e.net_e.reset_adam()
        e.step(LR)

    whole, second = _continuation(tmp_path, lambda seed: _engine(seed, 4, 50, 1000, ev=(4, 40), precision="bf16x3",
                                                                 after=after, weights=True), advance)
    assert second.e_trainable is True and second.net_e.adam_t == whole.net_e.adam_t == 5
    assert whole.validation_info() == second.validation_info() and second.validation_info()["records"] == 2
    assert second.balance_info()["updates"] == 5 and second.optimizer_info()["next_epoch"] == 2 * K
    a, b = whole.best_state_dict(), second.best_state_dict()
    assert a is not None and all(torch.equal(a[k], b[k]) for k in a)


def test_ev_with_batching_resampling_confgrad_supervised_continues(tmp_path):
    px, py = _points(3000, 4)

    def after(e):
        e.set_batching(batch_points=200, seed=9)
        e.set_conflict_free_gradients(True)
        e.set_resample_pool(px, py, (0.5 + px).astype(np.float32))

    def advance(e, i):
        if i in (5, 10):
            e.resample(k=1.0, c=1.0, seed=4)
        e.step(LR)

    whole, second = _continuation(tmp_path, lambda seed: _engine(seed, 4, 50, 1000, ev=(4, 40), precision="bf16x3",
                                                                 after=after, weights=True, sup=True), advance)
    assert second.batch_info()["draws"] == 2 * K and second._resample_calls == 2
    assert second.conflict_info()["steps"] == 2 * K


def test_hard_walls_pseudo_time_attention_continues(tmp_path):
    def before(e):
        e.set_hard_boundary(True)
        e.set_pseudo_time(dtau=0.5, every=4, pressure_dtau=2.0)

    whole, second = _continuation(tmp_path, lambda seed: _engine(
        seed, 6, 256, 320, precision="bf16x3", before=before, after=lambda e: e.set_residual_attention(eta=0.05, gamma=0.9)),
        _step)
    assert whole.pseudo_time_info() == second.pseudo_time_info() and second.pseudo_time_info()["refreshes"] >= 3


def test_lbfgs_continues_under_a_new_owner(tmp_path):
    def advance(e, i):
        e.lbfgs_step(max_iter=3, history_size=4, line_search_fn="strong_wolfe", owner=e)

    whole, second = _continuation(tmp_path, lambda seed: _engine(seed, 4, 50, 1000), advance, k=1)
    ls, ls2 = whole._lbfgs_state, second._lbfgs_state
    assert (ls.n_iter, ls.func_evals, ls.t, ls.prev_loss) == (ls2.n_iter, ls2.func_evals, ls2.t, ls2.prev_loss)
    assert ls.n_iter > 3                            # the history carried across the cut


def test_a_load_under_captured_graphs_replays_without_recapture(tmp_path, monkeypatch):
    monkeypatch.setenv("NSFNET_GRAPH", "1")
    e = _engine(5, 4, 50, 1000, after=lambda e: e.set_residual_attention(eta=0.05, gamma=0.9))
    for _ in range(3):
        e.step(LR)                                  # the first call captures, the others replay
    graphs = dict(e._graphs)
    assert len(graphs) == 1
    path = str(tmp_path / "state.bin")
    e.save_training_state(path)
    for _ in range(3):
        e.step(LR)
    first = _state(e)
    e.load_training_state(path)
    for _ in range(3):
        e.step(LR)
    _assert_same(first, _state(e))
    assert e._graphs == graphs                      # the same captured step served both times


def test_a_non_blocking_snapshot_holds_the_state_of_the_call(tmp_path):
    e = _engine(5, 4, 50, 1000, after=lambda e: e.set_residual_attention(eta=0.05, gamma=0.9))
    for _ in range(K):
        e.step(LR)
    want = _state(e, loss=False)
    path = str(tmp_path / "state.bin")
    e.save_training_state(path, wait=False)
    for _ in range(3):
        e.step(LR)
    info = e.training_state_info()                  # joins the writer
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    assert info["bytes"] == os.path.getsize(path) - sm.align256(16 + _header_len(path)) and info["stream_ms"] > 0.0
    other = _engine(77, 4, 50, 1000, after=lambda e: e.set_residual_attention(eta=0.05, gamma=0.9))
    other.load_training_state(path)
    _assert_same(want, _state(other, loss=False))


def _header_len(path):
    import struct
    with open(path, "rb") as f:
        return struct.unpack("<II", f.read(16)[8:])[1]
