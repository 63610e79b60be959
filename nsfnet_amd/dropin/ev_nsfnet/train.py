#!/usr/bin/env python3
"""ev-NSFnet staged training (reference flow: ev-NSFnet/train.py:74-224) on the MI355X engine.

    torchrun --nproc_per_node=N train.py --config configs/production.yaml [--dry-run] [--epochs-scale s]

One process per GPU; torchrun's RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* contract; backend "nccl"
(= RCCL on ROCm).  Every rank holds a contiguous shard of the points; one all-reduce per step."""
import argparse
import os

import numpy as np
import torch
import torch.distributed as dist

import cavity_data as cavity
import pinn_solver as psolver
from nsfnet_amd.pinn_solver import AdamHandle
from nsfnet_amd.schedule import LrSchedule
from config import ConfigManager
from logger import get_logger


def setup_distributed():
    if "RANK" not in os.environ or int(os.environ.get("WORLD_SIZE", "1")) < 2:
        os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
        return False
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
    dist.init_process_group(backend=os.environ.get("NSFNET_DIST_BACKEND", "nccl"))
    return True


def run_stages(PINN, stages, epochs_scale, rank, log, star=None, resume=None):
    """The staged schedule: per stage alpha_evm, then `epochs` (scaled) L-BFGS iterations or Adam updates at `lr`; an
    Adam stage with a scheduler or a warm-up runs under that device schedule, every count scaled like the epochs.
    resume: the `extra` of a loaded training state - the stages before its current_stage are skipped and that stage is
    entered at its next_epoch."""
    names = [st.name for st in stages]
    if resume is not None and resume.get("current_stage") not in names:
        raise ValueError("--resume: the state was saved in stage %r, the configuration has %s"
                         % (resume.get("current_stage"), names))
    for st in stages:
        start = 0
        if resume is not None:
            if st.name != resume["current_stage"]:
                continue
            start, resume = int(resume.get("next_epoch") or 0), None
        if rank == 0:
            log.stage(st.name, st.alpha, st.epochs, st.lr)
        PINN.current_stage = st.name
        PINN.set_alpha_evm(st.alpha)
        epochs = max(1, int(st.epochs * epochs_scale))
        if start >= epochs:         # the state was saved after the stage's last epoch
            continue
        if st.optimizer == "lbfgs":     # one epoch = one L-BFGS iteration of the main net, lr = step scale
            # max_eval: room for the line search (torch's default for max_iter = 1 is one evaluation)
            opt = torch.optim.LBFGS(PINN.net.parameters(), lr=st.lr, max_iter=1, max_eval=25,
                                    history_size=st.history_size,
                                    line_search_fn=None if st.line_search == "none" else st.line_search)
            PINN.train(num_epoch=epochs, lr=st.lr, optimizer=opt, start_epoch=start)
            PINN.set_optimizers(AdamHandle(st.lr))      # a later adam stage runs Adam again
        elif st.scheduler != "constant" or st.warmup_epochs > 0:    # lr is the base rate, the stage starts at epoch 0
            PINN.train(num_epoch=epochs, lr=st.lr, scheduler=LrSchedule(**st.schedule_args(epochs_scale)),
                       start_epoch=start)
        else:
            PINN.train(num_epoch=epochs, lr=st.lr, start_epoch=start)
        if rank == 0 and star is not None:
            PINN.evaluate(*star)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="configs/production.yaml")
    ap.add_argument("--dry-run", action="store_true")
    ap.add_argument("--epochs-scale", type=float, default=1.0)
    ap.add_argument("--data", default=None, help="DNS .mat (X_ref,Y_ref,U_ref,V_ref,P_ref)")
    ap.add_argument("--resume", default=None, metavar="FILE",
                    help="training state of training.checkpoint / save_training_state: continue its stage bit for bit")
    args = ap.parse_args()
    mgr = ConfigManager.from_file(args.config) if os.path.exists(args.config) else ConfigManager()
    cfg = mgr.config
    distributed = setup_distributed()
    rank = int(os.environ["RANK"])
    log = get_logger(cfg.experiment_name, rank=rank)
    if rank == 0:
        log.header("configuration")
        mgr.print_config()
        for i, st in enumerate(cfg.training.training_stages, 1):
            log.info("%02d | %-8s | alpha=%.3g | epochs=%s | lr=%.2e" % (i, st.name, st.alpha, format(st.epochs, ","), st.lr))
    if args.dry_run:
        return
    try:
        PINN = psolver.PysicsInformedNeuralNetwork(
            Re=cfg.physics.Re, layers=cfg.network.layers, layers_1=cfg.network.layers_1,
            hidden_size=cfg.network.hidden_size, hidden_size_1=cfg.network.hidden_size_1, N_f=cfg.training.N_f,
            alpha_evm=cfg.physics.alpha_evm, bc_weight=cfg.physics.bc_weight, eq_weight=cfg.physics.eq_weight,
            supervised_data_weight=cfg.supervision.loss_weight if cfg.supervision.enabled else 0.0)
        PINN.log_interval = cfg.training.log_interval
        loader = cavity.DataLoader(path="./datasets/", N_f=cfg.training.N_f, N_b=1000,
                                   sort_training_points=cfg.training.sort_training_points,
                                   sdf_weighting=cfg.training.sdf_weighting,
                                   coord_transform=cfg.training.coordinate_transform)
        ff = cfg.network.fourier_features
        if ff is not None:    # before any point set: every plan of the main net then sees the frozen sine first layer
            PINN.set_fourier_features(sigma=ff.sigma, seed=ff.seed)
        hb = cfg.training.hard_boundary
        if hb.enabled:        # before any point set: every plan of the main net is then created constrained
            PINN.set_coordinate_transform(loader.get_coord_scale())
            PINN.set_hard_boundary_constraints(lift_power=hb.lift_power, dataloader=loader)
        pt = cfg.training.pseudo_time
        if pt.enabled:        # before the collocation set: its plan is then created with the pseudo-time term
            PINN.set_pseudo_time_stepping(pt.dtau, pt.every, pressure_dtau=pt.pressure_dtau or None)
        PINN.set_boundary_data(X=loader.loading_boundary_data())
        if distributed:   # every rank must shard the SAME point set: rank 0 samples, the others receive
            pts = [loader.loading_training_data() + (loader.get_sdf_weights(),)] if rank == 0 else [None]
            dist.broadcast_object_list(pts, src=0)
            xf, yf, sdf = pts[0]
        else:
            xf, yf = loader.loading_training_data()
            sdf = loader.get_sdf_weights()
        PINN.set_coordinate_transform(loader.get_coord_scale())
        PINN.set_eq_training_data(X=(xf, yf), weights=sdf)
        rs = cfg.training.resampling
        if rs.enabled:    # the candidate pool: the same pipeline (LHS, coordinate map, sort, SDF weights) at N_f = pool_points
            pool_loader = cavity.DataLoader(path="./datasets/", N_f=rs.pool_points, N_b=1000,
                                            sort_training_points=cfg.training.sort_training_points,
                                            sdf_weighting=cfg.training.sdf_weighting,
                                            coord_transform=cfg.training.coordinate_transform)
            if rank == 0:
                pool_loader.loading_boundary_data()
                pool = [pool_loader.loading_training_data() + (pool_loader.get_sdf_weights(),)]
            else:
                pool = [None]
            if distributed:
                dist.broadcast_object_list(pool, src=0)
            xp, yp, sdfp = pool[0]
            PINN.set_resample_pool(X=(xp, yp), weights=sdfp)
            PINN.set_resampling(every=rs.every, k=rs.k, c=rs.c, seed=rs.seed)
        ref = args.data or "./data/cavity_Re%s_256_Uniform.mat" % cfg.physics.Re
        star = loader.loading_evaluate_data(ref) if os.path.exists(ref) else None
        sup = cfg.supervision
        if sup.enabled and sup.num_samples > 0 and star is not None:
            n = min(int(sup.num_samples), star[0].shape[0])
            idx = np.random.default_rng(0).choice(star[0].shape[0], size=n, replace=False)   # same on every rank
            PINN.set_supervised_data(tuple(a[idx] for a in star))
            PINN.set_supervised_loss_weight(sup.loss_weight)
        else:
            PINN.clear_supervised_data()
            PINN.set_supervised_loss_weight(0.0)
        lb = cfg.training.loss_balancing
        if lb.enabled:    # after the supervised weight: the balanced weights start at the configured ones
            PINN.set_loss_balancing(every=lb.every, beta=lb.beta)
        if cfg.training.conflict_free_gradients.enabled:    # the term gradients combined by the ConFIG rule
            PINN.set_conflict_free_gradients(True)
        bt = cfg.training.batching
        if bt.enabled:    # the collocation set is in place: it becomes the store the batches are drawn from
            PINN.set_batching(batch_points=bt.batch_points, seed=bt.seed)
        ra = cfg.training.residual_attention
        if ra.eta > 0:    # per-point attention weights on top of the SDF weights of the collocation set
            PINN.set_residual_attention(eta=ra.eta, gamma=ra.gamma, init=ra.init)
        gc = cfg.training.grad_clip
        if gc.max_norm > 0:   # global-norm clipping of every Adam update, on the device
            PINN.set_grad_clipping(max_norm=gc.max_norm)
        wf = cfg.training.weight_factorization
        if wf.enabled:        # W = diag(exp(s)) V on every layer of both nets; the optimizers act on (V, b, s)
            PINN.set_weight_factorization(mean=wf.mean, std=wf.std, seed=wf.seed)
        va = cfg.training.validation
        if va.enabled:
            if star is None:
                raise FileNotFoundError("training.validation needs the DNS file %s" % ref)
            # last: a change of the factorization would drop the best.  Every rank validates the whole grid
            PINN.set_validation_data(*star, every=va.every, metric=va.metric, keep_best=va.keep_best,
                                     patience=va.patience)
        es = cfg.training.early_stop
        if es is not None:    # an Adam stage that has stopped improving ends at a log point; the loop below goes on
            PINN.set_early_stopping(every=es.every, window=es.window, min_rel_improvement=es.min_rel_improvement,
                                    patience=es.patience, re_eff_tol=es.re_eff_tol, min_updates=es.min_updates,
                                    quantity=es.quantity, mode=es.mode)
        iv = cfg.training.identify_viscosity
        if iv is not None:    # the Reynolds number becomes a trainable scalar, pinned down by the supervised data
            PINN.set_viscosity_identification(re0=iv.re0, lr=iv.lr, re_bounds=(iv.re_min, iv.re_max))
        rc = cfg.training.re_continuation
        if rc is not None:    # the viscosity is ramped down to 1 / physics.Re while the stages train
            PINN.set_reynolds_continuation(rc.re_start, rc.updates, hold=rc.hold, shape=rc.shape, stairs=rc.stairs)
        fd = cfg.training.flow_diagnostics
        if fd is not None:    # which steady flow the net describes, recorded on the device; print_log adds the line
            PINN.set_flow_diagnostics(nx=fd.nx, ny=fd.ny, every=fd.every, eps=fd.eps)
        ck = cfg.training.checkpoint
        if ck.enabled:
            PINN.set_checkpointing(ck.path, ck.every)
        resume = None
        if args.resume:       # after every option and point set is attached: the state is unpacked into their tensors
            resume = PINN.load_training_state(args.resume)
        run_stages(PINN, cfg.training.training_stages, args.epochs_scale, rank, log, star, resume)
        if rank == 0:
            log.header("training completed")
    finally:
        if distributed and dist.is_initialized():
            dist.destroy_process_group()
        log.close()


if __name__ == "__main__":
    main()
