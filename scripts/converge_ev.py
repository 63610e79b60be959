"""Resumable ev-NSFnet convergence run against the DNS field (SURVEY 8d "converged field" gate).

The reference's production schedule (ev-NSFnet/configs/production.yaml: six Adam stages, alpha_evm
0.05 -> 0.002, lr 1e-3 -> 2e-6, 6x80 + 4x40 nets, 120 k LHS points, SDF weights) on ONE MI355X, in
slices that fit a 20-minute GPU job: every call runs stages [--first, --last] and writes the two
state_dicts + a JSON line per stage; the next call resumes from them (the reference re-creates Adam at
every stage start, so a stage boundary is an exact resume point for the optimiser; the lagged
viscosity state restarts from alpha*|e| as at the start of a run).

With --state FILE a slice may end anywhere: the run writes a training-state snapshot to FILE
every --state-every updates and where --max-steps cuts it, and a call that finds FILE continues from it bit for
bit, in the middle of its stage, with the state of every option below - the balanced weights, the draw counter,
the attention multipliers, the lagged viscosity, the schedule position, the validation ring and best weights, the
pseudo-time anchors, a resampled collocation set.  The call must be given the same options as the one that wrote FILE.

    python scripts/converge_ev.py --re 3000 --dns tests/golden/dns/cavity_Re3000_256_Uniform.mat \
        --out gpurun_out/conv_ev --first 1 --last 2 [--resume DIR] [--epochs-scale 0.5]
        [--resample-every 5000 --pool 1000000 --rs-k 1 --rs-c 1]   (residual-based resampling, off by default)
        [--balance-every 100 --balance-beta 0.1]   (adaptive boundary weight, off by default; restarts per call unless --state carries it)
        [--confgrad]   (conflict-free combination of the per-term gradients, off by default; stateless)
        [--batch-points 12000 --batch-seed 0]   (stochastic mini-batching, off by default; the draw counter restarts per call unless --state carries it)
        [--rba-eta 0.01 --rba-gamma 0.999]   (residual-based attention weights, off by default; lam restarts per call unless --state carries it)
        [--scheduler cosine --eta-min-factor 0.01 --warmup-epochs 1000]   (device learning-rate schedule of every stage,
                                                  off by default; counts scale with --epochs-scale, each stage starts at 0)
        [--grad-clip 1.0]   (global-norm gradient clipping of the Adam updates, off by default)
        [--validate-every 1000 --val-metric uv]   (error against the DNS field on the device every that many updates of
                                                  a stage, the stage's best weights kept: validation.jsonl,
                                                  net_best.pth / net_best_evm.pth; off by default)
        [--early-stop 1000 1e-3 --re-eff-tol 1e-3]   (device convergence monitor: a stage ends at a log point after three
                                                  windows of that many updates that improved the mean loss by less than
                                                  that fraction - or, with --re-eff-tol, moved the mean Re_eff by less;
                                                  the per-update curve goes to monitor.jsonl; off by default)
        [--identify-re 1000 1e-2]                 (the Reynolds number as a trainable scalar started at that value, its own
                                                  Adam rate on ln nu; every stage writes net.pth_visc (settings, state, nu) and
                                                  the estimate into stages.jsonl, a --resume slice continues from the sidecar
                                                  with its settings; off by default)
        [--re-continuation 400 500000]            (continuation in the Reynolds number: the viscosity is ramped geometrically
                                                  from 1 / 400 to 1 / --re over that many Adam updates, counted across the
                                                  stages; the position travels in --state: with --resume and no --state it
                                                  is refused; off by default)
        [--state FILE --state-every 50000 --max-steps 400000]   (training-state snapshots: continue from FILE when it
                                                  exists, write it every that many updates, end the call after that many
                                                  updates, anywhere in a stage)
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

STAGES = [(0.05, 500000, 1e-3), (0.03, 500000, 2e-4), (0.01, 500000, 4e-5),
          (0.005, 500000, 1e-5), (0.002, 500000, 2e-6), (0.002, 500000, 2e-6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--re", type=int, default=3000)
    ap.add_argument("--dns", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--resume", default=None, help="directory holding net.pth / net_evm.pth of the previous slice")
    ap.add_argument("--first", type=int, default=1)
    ap.add_argument("--last", type=int, default=6)
    ap.add_argument("--epochs-scale", type=float, default=1.0)
    ap.add_argument("--nf", type=int, default=120000)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=80)
    ap.add_argument("--resample-every", type=int, default=0,
                    help="> 0: redraw the collocation points from a pool every this many steps of each stage (DESIGN.md 7.1)")
    ap.add_argument("--pool", type=int, default=1000000, help="pool points (same pipeline as the collocation set)")
    ap.add_argument("--rs-k", type=float, default=1.0)
    ap.add_argument("--rs-c", type=float, default=1.0)
    ap.add_argument("--rs-seed", type=int, default=0)
    ap.add_argument("--balance-every", type=int, default=0, help="adaptive loss-weight balancing cadence (0: off)")
    ap.add_argument("--balance-beta", type=float, default=0.1)
    ap.add_argument("--confgrad", action="store_true",
                    help="conflict-free combination of the per-term gradients, ConFIG (DESIGN.md 7.8); not with --balance-every")
    ap.add_argument("--batch-points", type=int, default=0, help="stochastic mini-batching: points per Adam update (0: off)")
    ap.add_argument("--batch-seed", type=int, default=0)
    ap.add_argument("--rba-eta", type=float, default=0.0, help="residual-based attention: eta (0: off; DESIGN.md 7.5)")
    ap.add_argument("--rba-gamma", type=float, default=0.999)
    ap.add_argument("--rba-init", type=float, default=1.0)
    ap.add_argument("--scheduler", choices=("constant", "multistep", "step", "exponential", "cosine"), default="constant",
                    help="learning-rate schedule of every stage, on the device (DESIGN.md 7.6); lr0 = the stage's lr")
    ap.add_argument("--milestones", type=int, nargs="*", default=[], help="multistep: epochs of a stage at full scale")
    ap.add_argument("--gamma", type=float, default=0.1, help="multistep / step / exponential")
    ap.add_argument("--step-size", type=int, default=100000, help="step: epochs at full scale")
    ap.add_argument("--eta-min-factor", type=float, default=0.0, help="cosine: eta_min = this times the stage's lr")
    ap.add_argument("--warmup-epochs", type=int, default=0, help="linear warm-up, epochs at full scale")
    ap.add_argument("--warmup-start", type=float, default=0.0)
    ap.add_argument("--grad-clip", type=float, default=0.0, help="max global gradient norm of an Adam update (0: off)")
    ap.add_argument("--rwf", action="store_true",
                    help="random weight factorization W = diag(exp(s)) V of every layer of both nets (DESIGN.md 7.7); a "
                         "resumed slice takes up the net.pth_rwf the previous one wrote")
    ap.add_argument("--rwf-mean", type=float, default=0.5)
    ap.add_argument("--rwf-std", type=float, default=0.1)
    ap.add_argument("--rwf-seed", type=int, default=0)
    ap.add_argument("--hard-bc", type=int, nargs="?", const=2, default=0, metavar="M",
                    help="hard wall conditions by the output transform u = g + D N_u, v = D N_v with lift power M "
                         "(default 2; DESIGN.md 7.10); a resumed slice must be given the same M")
    ap.add_argument("--fourier", type=float, default=0.0, metavar="SIGMA",
                    help="> 0: random Fourier features of scale SIGMA as the main net's first layer, frozen (DESIGN.md "
                         "7.13); not with --hard-bc or --pseudo-time; a resumed slice must be given the same SIGMA")
    ap.add_argument("--fourier-seed", type=int, default=0)
    ap.add_argument("--pseudo-time", type=float, nargs=2, default=None, metavar=("DTAU", "EVERY"),
                    help="pseudo-time stepping of the equation loss: step DTAU, anchors refreshed every EVERY updates "
                         "(DESIGN.md 7.11); not with --resample-every or --batch-points")
    ap.add_argument("--pressure-dtau", type=float, default=0.0,
                    help="with --pseudo-time: the pseudo-time step of the continuity equation (0: none)")
    ap.add_argument("--validate-every", type=int, default=0,
                    help="> 0: validate against the DNS field on the device every this many updates of a stage and keep "
                         "the stage's best weights (DESIGN.md 7.9)")
    ap.add_argument("--val-metric", choices=("uv", "u", "v", "p", "p0"), default="uv", help="what `best` means")
    ap.add_argument("--early-stop", type=float, nargs=2, default=None, metavar=("WINDOW", "TOL"),
                    help="end a stage early on a loss plateau: window means over WINDOW updates, stale below a relative "
                         "improvement of TOL, three stale windows in a row (DESIGN.md 7.14)")
    ap.add_argument("--re-eff-tol", type=float, default=None, metavar="TOL",
                    help="also (or, without --early-stop, only) end a stage when the window mean of Re_eff moves by less "
                         "than TOL for three windows in a row (windows of --early-stop's WINDOW, else 1000 updates)")
    ap.add_argument("--identify-re", type=float, nargs="+", default=None, metavar=("RE0", "LR"),
                    help="learn the Reynolds number from the data (DESIGN.md 7.15): start at RE0, Adam rate LR on ln nu "
                         "(default 1e-2); not with --early-stop, --re-eff-tol, --pseudo-time or --confgrad")
    ap.add_argument("--re-continuation", type=float, nargs=2, default=None, metavar=("RE_START", "UPDATES"),
                    help="ramp the viscosity from 1 / RE_START to 1 / --re over UPDATES Adam updates (DESIGN.md 7.16); not "
                         "with --identify-re, --early-stop or --re-eff-tol")
    ap.add_argument("--flow-diag", type=int, nargs="+", default=None, metavar=("EVERY", "NX"),
                    help="EVERY [NX NY]: record the primary vortex, the counter-rotating area and the mass defect of the "
                         "net's field on an NX x NY grid (default 257 x 257) on the device every EVERY updates; the rows go "
                         "to flow.jsonl (DESIGN.md 7.17)")
    ap.add_argument("--state", default=None, metavar="FILE",
                    help="training-state file (DESIGN.md 7.12): continue from it when it exists, and write it")
    ap.add_argument("--state-every", type=int, default=0, help="updates between two non-blocking snapshots (0: only where the call ends)")
    ap.add_argument("--max-steps", type=int, default=0, help="> 0: end this call after that many updates, anywhere in a stage")
    a = ap.parse_args()
    state = None if a.state is None else os.path.abspath(a.state)
    from nsfnet_amd import ev_pinn_solver as es, cavity_data as cavity
    from nsfnet_amd.schedule import LrSchedule
    os.makedirs(a.out, exist_ok=True)
    dns = os.path.abspath(a.dns)
    res = None if a.resume is None else os.path.abspath(a.resume)
    os.chdir(a.out)
    np.random.seed(1234); torch.manual_seed(1234)       # same point set and (first slice) same init in every call
    P = es.PysicsInformedNeuralNetwork(
        Re=a.re, layers=a.layers, layers_1=4, hidden_size=a.hidden, hidden_size_1=40, N_f=a.nf, alpha_evm=0.05,
        bc_weight=10, eq_weight=1, supervised_data_weight=0.0,
        net_params=None if res is None else os.path.join(res, "net.pth"),
        net_params_1=None if res is None else os.path.join(res, "net_evm.pth"))
    P.log_interval = 20000
    from types import SimpleNamespace
    loader = cavity.EvDataLoader(path="./datasets/", N_f=a.nf, N_b=1000, sort_training_points=False,
                                 sdf_weighting=SimpleNamespace(enabled=True, min_weight=0.2, decay=5.0),
                                 coord_transform=False)
    if a.fourier > 0:                                   # before any point set is attached (the same seed redraws the same B)
        P.set_fourier_features(sigma=a.fourier, seed=a.fourier_seed)
    if a.hard_bc:                                       # before any point set is attached
        P.set_coordinate_transform(loader.get_coord_scale())
        P.set_hard_boundary_constraints(lift_power=a.hard_bc, dataloader=loader)
    if a.pseudo_time is not None:                       # before the collocation set is attached
        P.set_pseudo_time_stepping(a.pseudo_time[0], int(a.pseudo_time[1]), pressure_dtau=a.pressure_dtau or None)
    P.set_boundary_data(X=loader.loading_boundary_data())
    xf, yf = loader.loading_training_data()
    P.set_coordinate_transform(loader.get_coord_scale())
    P.set_eq_training_data(X=(xf, yf), weights=loader.get_sdf_weights())
    if a.resample_every > 0:      # drawn after the collocation set: the set and the init are those of the run without
        pool = cavity.EvDataLoader(path="./datasets/", N_f=a.pool, N_b=1000, sort_training_points=False,
                                   sdf_weighting=SimpleNamespace(enabled=True, min_weight=0.2, decay=5.0),
                                   coord_transform=False)
        pool.loading_boundary_data()
        P.set_resample_pool(X=pool.loading_training_data(), weights=pool.get_sdf_weights())
        P.set_resampling(every=a.resample_every, k=a.rs_k, c=a.rs_c, seed=a.rs_seed)
    P.clear_supervised_data(); P.set_supervised_loss_weight(0.0)
    if a.balance_every > 0:
        P.set_loss_balancing(every=a.balance_every, beta=a.balance_beta)
    if a.confgrad:
        P.set_conflict_free_gradients(True)
    if a.batch_points > 0:
        P.set_batching(batch_points=a.batch_points, seed=a.batch_seed)
    if a.rba_eta > 0:
        P.set_residual_attention(eta=a.rba_eta, gamma=a.rba_gamma, init=a.rba_init)
    if a.grad_clip > 0:
        P.set_grad_clipping(a.grad_clip)
    if a.rwf:
        side = None if res is None else os.path.join(res, "net.pth_rwf")
        if side is not None and os.path.exists(side):       # carry the trained scale factors across slices
            P.set_weight_factorization(factors=torch.load(side, map_location="cpu", weights_only=True))
        else:
            P.set_weight_factorization(mean=a.rwf_mean, std=a.rwf_std, seed=a.rwf_seed)
    monitor = a.early_stop is not None or a.re_eff_tol is not None
    if monitor:                                         # every stage start resets it; the ring keeps the stage's curve
        P.set_early_stopping(window=1000 if a.early_stop is None else int(a.early_stop[0]),
                             min_rel_improvement=None if a.early_stop is None else a.early_stop[1],
                             re_eff_tol=a.re_eff_tol, history=1 << 16)
    if a.flow_diag is not None:
        if len(a.flow_diag) not in (1, 3):
            ap.error("--flow-diag takes EVERY or EVERY NX NY")
        nx, ny = a.flow_diag[1:] if len(a.flow_diag) == 3 else (257, 257)
        P.set_flow_diagnostics(nx=nx, ny=ny, every=a.flow_diag[0], history=1 << 16)
    if a.identify_re is not None:
        if len(a.identify_re) > 2:
            ap.error("--identify-re takes RE0 and, optionally, LR")
        P.set_viscosity_identification(re0=a.identify_re[0], lr=a.identify_re[1] if len(a.identify_re) > 1 else 1e-2)
        if res is not None:                             # carry the estimate and its optimiser state across slices
            P._load_viscosity(os.path.join(res, "net.pth"))
    if a.re_continuation is not None:                   # the position counts on across the stages
        if res is not None and state is None:
            ap.error("--re-continuation with --resume needs --state: the ramp's position travels in the training-state "
                     "file only, and a resumed slice without it would restart the trained net at RE_START")
        P.set_reynolds_continuation(a.re_continuation[0], int(a.re_continuation[1]))
    P.save = lambda *args, **kw: None                   # no per-10 000-step checkpoints: one per stage below
    star = loader.loading_evaluate_data(dns)
    first, start, left = a.first, 0, a.max_steps if a.max_steps > 0 else None
    if state is not None:
        P.set_checkpointing(state, a.state_every if a.state_every > 0 else 1 << 62)
    resumed = state is not None and os.path.exists(P.engine._state_path(state))
    if resumed:       # the stage the file was cut in, entered at its next epoch
        first = int(es._eng._state_file.read_header(P.engine._state_path(state))["extra"]["current_stage"].split()[-1])
    flow_seen = 0                                       # flow records already in flow.jsonl
    for k in range(first, a.last + 1):
        alpha, epochs, lr = STAGES[k - 1]
        n = max(1, int(epochs * a.epochs_scale))
        P.current_stage = "Stage %d" % k
        P.set_alpha_evm(alpha)
        if a.validate_every > 0:                        # per stage: t counts the stage's updates, the best is the stage's
            P.set_validation_data(*star, every=a.validate_every, metric=a.val_metric,
                                  history=max(1, n // a.validate_every))
        if resumed:   # every option is attached as in the call that wrote the file
            start, resumed = int(P.load_training_state(state)["next_epoch"]), False
            if a.flow_diag is not None:                 # the restored ring's rows were written by the call that made them
                flow_seen = P.engine.flow_info()["records"]
            if start >= n:
                start = 0
                continue
        stop = None if left is None else start + left
        t0 = time.time()
        sched = None
        if a.scheduler != "constant" or a.warmup_epochs > 0:
            c = lambda v, lo: max(lo, int(v * a.epochs_scale))
            sched = LrSchedule(a.scheduler, milestones=[c(m, 0) for m in a.milestones], gamma=a.gamma,
                               step_size=c(a.step_size, 1), t_max=n, eta_min=a.eta_min_factor * lr,
                               warmup_epochs=c(a.warmup_epochs, 0), warmup_start=a.warmup_start)
        P.train(num_epoch=n, lr=lr, scheduler=sched, start_epoch=start, stop_epoch=stop)
        torch.cuda.synchronize()
        if stop is not None and stop < n:               # the call's budget ends inside the stage: the snapshot is written
            P.engine.training_state_info()
            print("SLICE", json.dumps(dict(stage=k, next_epoch=stop, steps=n, state=state)), flush=True)
            return
        if left is not None:
            left -= n - start
        ran = n - start
        if monitor:                                     # a stage that stopped early ran fewer (the monitor counts the stage's updates)
            ran = max(1, min(ran, P.engine.monitor_info()["updates"] - start))
        start = 0
        dt = time.time() - t0
        eu, ev = P.evaluate(*star)[:2]
        rec = dict(stage=k, alpha_evm=alpha, lr=lr, steps=n, seconds=round(dt, 1), ms_per_step=round(1e3 * dt / ran, 4),
                   loss=float(P.loss), loss_b=float(P.loss_b), loss_e=float(P.loss_e),
                   err_u=float(eu), err_v=float(ev), Re=a.re, net="%dx%d+4x40" % (a.layers, a.hidden), N_f=a.nf,
                   precision=os.environ.get("NSFNET_PRECISION", "fp32"),
                   resample=(dict(every=a.resample_every, pool=a.pool, k=a.rs_k, c=a.rs_c, seed=a.rs_seed)
                             if a.resample_every > 0 else None),
                   balance=(dict(every=a.balance_every, beta=a.balance_beta, lambda_b=P.lam_b())
                            if a.balance_every > 0 else None),
                   confgrad=(P.engine.conflict_info() if a.confgrad else None),
                   batching=(dict(batch_points=a.batch_points, seed=a.batch_seed) if a.batch_points > 0 else None),
                   attention=(dict(eta=a.rba_eta, gamma=a.rba_gamma, init=a.rba_init,
                                   **{k_: v for k_, v in P.engine.attention_info().items()
                                      if k_ in ("lam_min", "lam_mean", "lam_max", "loss_e", "skipped")})
                              if a.rba_eta > 0 else None),
                   optimizer=({k_: (v if k_ != "schedule" else (None if v is None else v.key()))
                               for k_, v in P.engine.optimizer_info().items()}
                              if P.engine.optimizer_info() is not None else None))
        if a.validate_every > 0:
            info = P.engine.validation_info()
            rec.update(best_metric=info["best_metric"], best_t=info["best_t"], val_metric=a.val_metric)
            with open("validation.jsonl", "a") as fh:
                for row in P.validation_history().tolist():
                    fh.write(json.dumps(dict(zip(("t", "e_u", "e_v", "e_p", "e_p0", "metric", "improved", "n_p"), row),
                                             stage=k)) + "\n")
            best = P.best_state_dict()
            if best is not None:
                torch.save(best, "net_best.pth")
                torch.save(P.engine.best_state_dict_e(), "net_best_evm.pth")
        if monitor:
            info = P.engine.monitor_info()
            rec.update(early_stop=dict(updates=info["updates"], reasons=info["reasons"], stopped=info["should_stop"],
                                       window_mean=info["window_mean"], window_mean_re=info["window_mean_re"]))
            with open("monitor.jsonl", "a") as fh:
                for row in P.monitor_history().tolist():
                    fh.write(json.dumps(dict(zip(("t", "loss", "loss_e", "loss_b", "loss_s", "eq1", "eq2", "eq3", "eq4",
                                                  "vis_mean", "Re_eff", "stop"), row), stage=k)) + "\n")
        if a.flow_diag is not None:
            info = P.engine.flow_info()
            rec.update(flow=info["last"])
            new = info["records"] - flow_seen           # the ring runs on across the stages: this stage's rows
            if new > 0:
                from nsfnet_amd.engine import FLOW_ROW
                with open("flow.jsonl", "a") as fh:
                    for row in P.flow_history()[-new:].tolist():
                        fh.write(json.dumps(dict(zip(FLOW_ROW, row), stage=k)) + "\n")
            flow_seen = info["records"]
        if a.identify_re is not None:
            info = P.engine.viscosity_info()
            rec.update(viscosity={k_: info[k_] for k_ in ("Re", "nu", "grad", "updates", "skipped")})
        if a.re_continuation is not None:
            info = P.engine.continuation_info()
            rec.update(re_continuation={k_: info[k_] for k_ in ("t", "s", "Re_t", "nu_t", "cap_t", "done")})
        with open("stages.jsonl", "a") as fh:
            fh.write(json.dumps(rec) + "\n")
        print("STAGE", json.dumps(rec), flush=True)
        torch.save(P.net.state_dict(), "net.pth")
        torch.save(P.net_1.state_dict(), "net_evm.pth")
        P.save_weight_factors("net.pth")                 # net.pth_rwf with --rwf, nothing without
        P.save_hard_boundary("net.pth")                  # net.pth_hardbc with --hard-bc, nothing without
        P.save_viscosity("net.pth")                      # net.pth_visc with --identify-re, nothing without
        if left is not None and left <= 0:               # the call's budget ended with the stage
            return


if __name__ == "__main__":
    main()
