// C ABI (include/nsfnet_pinn.h) over the HIP kernels.  Host-side only: argument
// checking, workspace carving and launches.  No device allocation happens here.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <atomic>
#include <new>

#include "../../include/nsfnet_pinn.h"
#include "kernels.h"
#include "optim.h"
#include "rwf.h"
#include "visc_sched.h"

static_assert((int)PINN_FLD_COUNT == (int)FLD_COUNT, "field plane enum mismatch");

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, const char* a = "", long b = 0) {
  snprintf(g_err, sizeof(g_err), fmt, a, b);
  return code;
}
static int hipfail(int rc, const char* what) {
  if (rc == -1000) return fail(-22, "%s: unsupported hidden width or spill layout (code %ld)", what, (long)rc);
  return fail(rc, "%s: HIP error %ld", what, (long)-rc);
}

// The environment switches, all read here.  read_switches() runs at every plan creation, and for tile_cols at net
// creation and in pinn_net_set_precision: callers change the variables between calls in one process.
struct Switches {
  int sched_f, sched_b;   // $PINN_FWD_SCHED / $PINN_BWD_SCHED, each defaulting to $PINN_SCHED (default 2)
  int wsplit, fuse;       // $PINN_WSPLIT, $PINN_FUSE (default 1; 0 opts out)
  int stagger;            // $PINN_STAGGER (default 0)
  int s0_skip32;          // $PINN_S0_SKIP32 (default 1; 0 opts out)
  int verbose;            // $PINN_VERBOSE
  int tile_cols;          // $PINN_TILE_COLS = 64 | 128 overrides pick_wide (hidden 128 / 256 only)
  int hbc_split;          // $PINN_HBC_SPLIT (default 0; 1: a constrained plan may take the role-split / fused sweeps)
  int ptime_split;        // $PINN_PTIME_SPLIT (default 0; 1: a pseudo-time plan may take the role-split / fused sweeps)
  int ff_split;           // $PINN_FF_SPLIT (default 0; 1: a plan over a frozen sine first layer may take the role-split / fused sweeps)
};
static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
static Switches read_switches() {
  const int sched = env_int("PINN_SCHED", 2);
  return {env_int("PINN_FWD_SCHED", sched), env_int("PINN_BWD_SCHED", sched), env_int("PINN_WSPLIT", 1),
          env_int("PINN_FUSE", 1), env_int("PINN_STAGGER", 0), env_int("PINN_S0_SKIP32", 1),
          env_int("PINN_VERBOSE", 0), env_int("PINN_TILE_COLS", 0), env_int("PINN_HBC_SPLIT", 0),
          env_int("PINN_PTIME_SPLIT", 0), env_int("PINN_FF_SPLIT", 0)};
}

// precision of a kernel family: 0 = fp32-input MFMA (exact fp32), 1 = bf16x3 split, 2 = plain bf16
// What a net shares with the plans created over it (each plan keeps a copy of pinn_net_s): the first-layer kind as it
// is NOW, so that a launch can refuse a plan whose copy predates a change.  Reference counted: it outlives whichever of
// the net and its plans is destroyed first.
struct NetShared { std::atomic<int> refs, first_layer; };
static void shared_release(NetShared* s) { if (s && s->refs.fetch_sub(1) == 1) delete s; }
struct pinn_net_s {
  int n_out, L, H, HP;
  int wide;   // 64-column tile kernels (always for HP > 256; pick_wide for HP 128/256)
  int prec_fwd, prec_bwd, prec_dw;
  int first_layer;      // PINN_FIRST_LAYER_TANH | PINN_FIRST_LAYER_SINE (pinn_net_set_first_layer); a plan's copy: at its creation
  NetShared* shared;
};
static bool is_ff(const pinn_net_s& n) { return n.first_layer == PINN_FIRST_LAYER_SINE; }
static int terms_of(int prec) { return prec == 1 ? 3 : 1; }
// 64-column-tile kernels: always for HP > 256; for HP == 256 in fp32 mode they are also the faster
// choice (two workgroups per CU overlap each other's epilogue and MFMA phases).
static int pick_wide(const pinn_net_s* n) {
  if (n->HP > 256) return 1;
  if (n->HP != 256 && n->HP != 128) return 0;
  const bool fp32 = !n->prec_fwd && !n->prec_bwd && !n->prec_dw;
  // measured (6x256, 360k pts): fp32 26.2 vs 29.6 ms/step in favour of 64-column tiles; bf16x3 13.4 vs 12.6 ms
  // against them.  PINN_TILE_COLS=64|128 overrides the choice (HP 128/256 only).
  const int force = read_switches().tile_cols;
  if (force == 64) return 1;
  if (force == 128) return 0;
  return fp32 && n->HP == 256;
}

// Kernel families.  A plan's role (forward with / without saved activations, reverse sweep, dW, fused sweeps) runs
// one of them, chosen once by resolve_plan; launches, LDS sizes and reported names switch over the value.
enum Family { FAM_NONE = 0, FAM_FP32, FAM_FP32_WIDE, FAM_BF16, FAM_BF16_WIDE, FAM_PIPE, FAM_SPLIT, FAM_WSPLIT, FAM_FUSED };
// names as pinn_plan_kernel reports them: {forward, reverse sweep, dW}.  A fused plan keeps reporting its forward and
// reverse roles (fwd_split_kernel / bwd_split_kernel) for kernels 0 and 1, not fwdbwd_split_kernel: scripts and tests
// key on those names, and the two kernels are still what forward-only and PINN_FUSE=0 calls launch.
static constexpr const char* FAMILY_NAMES[][3] = {
    {nullptr, nullptr, nullptr},
    {"fwd_kernel", "bwd_kernel", "dw_kernel"},
    {"fwd_wide_kernel", "bwd_wide_kernel", "dw_wide_kernel"},
    {"fwd_bf16_kernel", "bwd_bf16_kernel", "dw_bf16_kernel"},
    {"fwd_bf16_wide_kernel", "bwd_bf16_wide_kernel", "dw_bf16_wide_kernel"},
    {"fwd_pipe_kernel", "bwd_pipe_kernel", nullptr},
    {"fwd_split_kernel", "bwd_split_kernel", nullptr},
    {"fwd_wsplit_kernel", "bwd_wsplit_kernel", nullptr},
    {"fwdbwd_split_kernel", "fwdbwd_split_kernel", nullptr},
};
// The spill layouts (spill.h) each family's kernels implement in residual mode: {S the forward writes, S the reverse
// sweep reads and Z-bar it writes, S and Z-bar the dW kernel reads}.  resolve_plan checks every role of a plan against
// this table and the launchers check again what they are handed; value mode is SPILL_CLASSIC in every 8-wave family.
static constexpr unsigned FAMILY_SPILLS[][3] = {
    {0, 0, 0},
    {IN_CLASSIC | IN_SKIP0, IN_CLASSIC | IN_SKIP0, IN_CLASSIC | IN_SKIP0},
    {IN_CLASSIC | IN_SKIP0, IN_CLASSIC | IN_SKIP0, IN_CLASSIC | IN_SKIP0},
    {IN_CLASSIC, IN_CLASSIC, IN_CLASSIC | IN_P24_COMPACT},      // (dw_bf16 reads the compact layout at hidden 256 / 128 columns)
    {IN_CLASSIC | IN_P24_WIDE, IN_CLASSIC | IN_P24_WIDE, IN_CLASSIC | IN_P24_WIDE},
    {IN_CLASSIC, IN_CLASSIC, 0},
    {IN_P24_COMPACT, IN_P24_COMPACT, 0},
    {IN_P24_WIDE, IN_P24_WIDE, 0},
    {IN_P24_COMPACT, IN_P24_COMPACT, 0},
};
// The variants (launch_dispatch.h) each family's sweeps have in residual mode, by the names its launchers dispatch on.
// resolve_plan keeps a sweep out of a family that lacks the plan's variant and checks every role again once the plan
// is resolved; the launchers refuse what is outside their mask.  The dW kernels serve every variant.
static constexpr unsigned FAMILY_VARIANTS[] = {
    0,
    VARIANTS_WAVE8, VARIANTS_WAVE8, VARIANTS_WAVE8, VARIANTS_WAVE8,      // fp32, fp32 wide, bf16, bf16 wide
    VARIANTS_PIPE,
    VARIANTS_SPLIT, VARIANTS_SPLIT, VARIANTS_SPLIT,                      // role-split, wide role-split, fused
};
static const char* variant_name(unsigned bit) {
  return bit == VAR_FF ? "frozen-sine" : bit == VAR_HBC_PT ? "constrained pseudo-time" : bit == VAR_PT ? "pseudo-time" : bit == VAR_HBC ? "constrained" : "plain";
}
// the 8-wave family of one precision on this net: the only place precision and tile geometry are weighed
static Family base_family(const pinn_net_s& n, int prec) {
  return prec ? (n.HP > 256 ? FAM_BF16_WIDE : FAM_BF16) : n.wide ? FAM_FP32_WIDE : FAM_FP32;
}

enum { ROLE_FWD_SAVE = 0, ROLE_FWD, ROLE_BWD, ROLE_DW, ROLE_FUSED, ROLE_COUNT };
static constexpr int ROLE_SPILL_COL[ROLE_COUNT] = {0, -1, 1, 2, 0};      // the role's column of FAMILY_SPILLS (ROLE_FWD saves nothing)
struct Role {
  Family family;      // FAM_NONE: the plan has no such kernel (ROLE_FUSED)
  int grid;           // workgroups (ROLE_DW: the group count; its launcher derives the grid from DwArgs)
  size_t lds;         // dynamic LDS bytes
  const char* name;
};

struct pinn_plan_s {
  pinn_net_s net;
  long n;
  int streams, ntiles, npad;
  int groups;            // dW slabs per layer
  int stagger;           // $PINN_STAGGER, read once at plan creation
  Role role[ROLE_COUNT];
  Spill spill;           // how the sweeps spill S and Z-bar, and what their readers recompute instead (spill.h)
  HardBc hbc;            // hard wall conditions (kind 0: none); resolve_plan says which families a constrained plan runs
  int ptime;             // a pseudo-time plan (pinn_plan_create_pseudo_time); resolve_plan says which families it runs
  const float* anchor;   // its anchors [3][npad] (pinn_plan_set_pseudo_time; NULL: unset, residual calls are refused)
  float sigma, sigma_p;  // its rates
  const float* nu_dev;   // viscosity identification (pinn_plan_set_viscosity; residual plans): the fp32 read in place of 1 / Re, or NULL
  float* lap;            // and the planes [2][npad] the forward leaves Lap u, Lap v in, or NULL
  const float* cap_dev;  // Reynolds-number continuation (pinn_plan_set_viscosity_cap): the fp32 read in place of vis_t0, or NULL
  // workspace offsets in bytes
  size_t off_partials, off_oadj, off_sg, off_slabs, off_S, off_Zb, bytes_fwd, bytes_all;
};

// compute units of the CURRENT device (queried per plan: no cached value, a process may drive several devices)
static int num_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) == hipSuccess &&
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
    return n;
  (void)hipGetLastError();
  return 256;   // MI355X (also what a device-less host sizes workspaces for)
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// per role: the LDS bytes of a family, and its launch (args.configure = 1: set the dynamic-LDS attribute of exactly
// the kernel a launch would pick, pinn_plan_create's configure pass)
static size_t fwd_lds(Family f, const pinn_net_s& n) {
  switch (f) {
    case FAM_FP32: return fwd_lds_bytes(n.HP);
    case FAM_FP32_WIDE: return fwd_wide_lds_bytes(n.HP);
    case FAM_BF16: return fwd_bf16_lds_bytes(n.HP, n.L, n.wide ? 64 : 128);
    case FAM_BF16_WIDE: return fwd_bf16_wide_lds_bytes(n.HP, n.L);
    case FAM_PIPE: return fwd_pipe_lds_bytes(n.HP, n.L);
    case FAM_SPLIT: return fwd_split_lds_bytes(n.HP, n.L);
    case FAM_WSPLIT: return fwd_wsplit_lds_bytes(n.HP);
    default: return 0;
  }
}
static size_t bwd_lds(Family f, const pinn_net_s& n) {
  switch (f) {
    case FAM_FP32: return bwd_lds_bytes(n.HP, n.L);
    case FAM_FP32_WIDE: return bwd_wide_lds_bytes(n.HP, n.L);
    case FAM_BF16: return bwd_bf16_lds_bytes(n.HP, n.L, n.wide ? 64 : 128);
    case FAM_BF16_WIDE: return bwd_bf16_wide_lds_bytes(n.HP, n.L);
    case FAM_PIPE: return bwd_pipe_lds_bytes(n.HP, n.L);
    case FAM_SPLIT: return bwd_split_lds_bytes(n.HP, n.L);
    case FAM_WSPLIT: return bwd_wsplit_lds_bytes(n.HP, n.L);
    default: return 0;
  }
}
static size_t dw_lds(Family f, const pinn_net_s& n) {
  switch (f) {
    case FAM_FP32: return dw_lds_bytes(n.HP);
    case FAM_FP32_WIDE: return dw_wide_lds_bytes();
    case FAM_BF16: return dw_bf16_lds_bytes(n.HP);
    case FAM_BF16_WIDE: return dw_bf16_wide_lds_bytes();
    default: return 0;
  }
}
static int run_fwd(const pinn_plan_s* plan, const Role& r, const FwdArgs& a, hipStream_t s) {
  const pinn_net_s& n = plan->net;
  const int NS = plan->streams, terms = terms_of(n.prec_fwd);
  switch (r.family) {
    case FAM_FP32: return launch_fwd(n.HP, NS, a, r.grid, s);
    case FAM_FP32_WIDE: return launch_fwd_wide(n.HP, NS, a, r.grid, s);
    case FAM_BF16: return launch_fwd_bf16(n.HP, NS, terms, n.wide ? 64 : 128, a, r.grid, s);
    case FAM_BF16_WIDE: return launch_fwd_bf16_wide(n.HP, NS, terms, a, r.grid, s);
    case FAM_PIPE: return launch_fwd_pipe(n.HP, terms, a, r.grid, s);
    case FAM_SPLIT: return launch_fwd_split(n.HP, terms, a, r.grid, s);
    case FAM_WSPLIT: return launch_fwd_wsplit(n.HP, terms, a, r.grid, s);
    default: return -1000;
  }
}
static int run_bwd(const pinn_plan_s* plan, const BwdArgs& a, hipStream_t s) {
  const pinn_net_s& n = plan->net;
  const Role& r = plan->role[ROLE_BWD];
  const int NS = plan->streams, terms = terms_of(n.prec_bwd);
  switch (r.family) {
    case FAM_FP32: return launch_bwd(n.HP, NS, a, r.grid, s);
    case FAM_FP32_WIDE: return launch_bwd_wide(n.HP, NS, a, r.grid, s);
    case FAM_BF16: return launch_bwd_bf16(n.HP, NS, terms, n.wide ? 64 : 128, a, r.grid, s);
    case FAM_BF16_WIDE: return launch_bwd_bf16_wide(n.HP, NS, terms, a, r.grid, s);
    case FAM_PIPE: return launch_bwd_pipe(n.HP, terms, a, r.grid, s);
    case FAM_SPLIT: return launch_bwd_split(n.HP, terms, a, r.grid, s);
    case FAM_WSPLIT: return launch_bwd_wsplit(n.HP, terms, a, r.grid, s);
    default: return -1000;
  }
}
static int run_dw(const pinn_plan_s* plan, const DwArgs& d, hipStream_t s) {
  const pinn_net_s& n = plan->net;
  const int NS = plan->streams, terms = terms_of(n.prec_dw);
  switch (plan->role[ROLE_DW].family) {
    case FAM_FP32: return launch_dw(n.HP, NS, d, s);
    case FAM_FP32_WIDE: return launch_dw_wide(n.HP, NS, d, s);
    case FAM_BF16: return launch_dw_bf16(n.HP, NS, terms, n.wide ? 64 : 128, d, s);
    case FAM_BF16_WIDE: return launch_dw_bf16_wide(n.HP, NS, terms, d, s);
    default: return -1000;
  }
}
static int run_fused(const pinn_plan_s* plan, const FwdArgs& fa, const BwdArgs& ba, hipStream_t s) {
  return launch_fwdbwd_split(plan->net.HP, terms_of(plan->net.prec_fwd), fa, ba, plan->role[ROLE_FUSED].grid, s);
}

// Resolves a plan: tiles, one Role per kernel role, the spill format and the workspace layout.  Pure host arithmetic
// (no HIP call) on the net, the point and stream counts, the compute-unit count and the switches.
static int resolve_plan(pinn_plan_s* p, const pinn_net_s& net, long n_points, int streams, int cus, const Switches& sw_in,
                        const HardBc& hbc = HardBc{}, bool ptime = false) {
  // Which family has which variant of the point stage - hard walls, the pseudo-time term, both, the frozen sine first
  // layer - is FAMILY_VARIANTS: every family but the pipelined schedule has all of them.  By default a plan of any
  // variant but the plain one resolves as PINN_SCHED=0 PINN_WSPLIT=0 PINN_FUSE=0 would, whatever those switches say.
  // One switch per variant opts out of that, each read by its own plans only: $PINN_PTIME_SPLIT=1 for a pseudo-time plan
  // (constrained or not), $PINN_HBC_SPLIT=1 for any other constrained plan, $PINN_FF_SPLIT=1 for a residual plan over a
  // sine net.  Such a plan keeps what the other switches give it, except that a sweep which would run the pipelined
  // kernels (PINN_SCHED=1, an incomplete role-split pair, an fp32 dW) runs the 8-wave kernel instead.  The spill format
  // follows from the resolved families as for any other plan.  A sine net has no variant with walls or pseudo-time, and
  // its layer 0 holds the a-streams, which no reader recomputes: its 8-wave plans are SPILL_CLASSIC in every precision,
  // and it keeps the role-split sweeps only where BOTH land in the same role-split family - the complete hidden-256 pair
  // with the bf16 dW (fused where that holds; the compact layout recomputes layer 0, layer0_sine) or the wide pair (the
  // a-streams stay in layer 0's slot, in the 24-bit format) - so no plan mixes layouts.
  Switches sw = sw_in;
  const bool ff = is_ff(net);
  if (ff && (hbc.kind || ptime))
    return fail(-22, "pinn_plan_create: a net with the frozen sine first layer has no %s variant", hbc.kind ? "hard-wall (constrained)" : "pseudo-time");
  const bool keep_split = ff ? sw.ff_split != 0 : ptime ? sw.ptime_split != 0 : hbc.kind && sw.hbc_split != 0;
  if ((hbc.kind || ptime || ff) && !keep_split) { sw.sched_f = sw.sched_b = 0; sw.wsplit = 0; sw.fuse = 0; }
  p->net = net;
  p->hbc = hbc;
  p->ptime = ptime; p->anchor = nullptr; p->sigma = p->sigma_p = 0.f;
  p->nu_dev = nullptr; p->lap = nullptr; p->cap_dev = nullptr;
  p->n = n_points; p->streams = streams;
  const bool wide = net.wide != 0;
  const int per_tile = wide ? (streams == 4 ? 16 : 64) : (streams == 4 ? 32 : 128);
  p->ntiles = (int)((n_points + per_tile - 1) / per_tile);
  p->npad = p->ntiles * per_tile;
  const int HP = net.HP, L = net.L, NW = HP / 32;
  auto bpc = [&](size_t lds) {
    int b = (int)(PINN_LDS_MAX / lds);
    int bw = NW >= 8 ? (wide && NW == 8 ? 2 : 1) : 8 / NW;
    if (b > bw) b = bw;
    return b < 1 ? 1 : b;
  };
  auto role = [&](int which, Family f, int grid, size_t lds, int name_col) {
    p->role[which] = Role{f, grid, lds, FAMILY_NAMES[f][name_col]};
  };
  // the 8-wave kernels: what forward-only calls (save = 0) and value plans always run.  A plan whose 8-wave forward
  // or reverse kernel does not fit in LDS is refused, whatever schedule its sweeps would take.
  const Family f8 = base_family(net, net.prec_fwd), b8 = base_family(net, net.prec_bwd), d8 = base_family(net, net.prec_dw);
  const size_t lds_f = fwd_lds(f8, net), lds_b = bwd_lds(b8, net), lds_d = dw_lds(d8, net);
  if (lds_b > PINN_LDS_MAX || lds_f > PINN_LDS_MAX) return fail(-22, "pinn_plan_create: this depth x width needs more than 160 KiB of LDS%s");
  int grid_f = cus * bpc(lds_f);
  if (grid_f > p->ntiles) grid_f = p->ntiles;
  int grid_b = cus * bpc(lds_b);
  if (grid_b > p->ntiles) grid_b = p->ntiles;
  const int grid_fp = cus < (p->ntiles + 1) / 2 ? cus : (p->ntiles + 1) / 2;   // pipelined / role-split kernels: pairs of tiles
  // Schedule of the hidden-256 bf16 sweeps in residual mode: 0 = 8-wave kernels (fwd_bf16 / bwd_bf16), 1 = one wave
  // per SIMD, two tiles per wave (fwd_bf16_pipe / bwd_bf16_pipe), 2 = two wave groups in opposite phases
  // (fwd_bf16_split / bwd_bf16_split).  $PINN_FWD_SCHED / $PINN_BWD_SCHED choose per sweep, $PINN_SCHED both.
  // Default 2.  Round-2 measurements at 6x256 / 360k points (ms): forward 2.84 / 2.65 / 2.47, reverse sweep
  // 3.75 / 3.40 / 3.22 - the schedules end close to each other because all of them wait on the spill traffic
  // (DESIGN.md section 4.3).
  const bool pipe_shape = HP == 256 && !wide && streams == 4 && L >= 2;
  int sf = sw.sched_f, sb = sw.sched_b;
  if (!pipe_shape || !net.prec_fwd) sf = 0;
  if (!pipe_shape || !net.prec_bwd) sb = 0;
  if (sf == 2 && fwd_lds(FAM_SPLIT, net) > PINN_LDS_MAX) sf = 1;
  if (sf == 1 && fwd_lds(FAM_PIPE, net) > PINN_LDS_MAX) sf = 0;
  if (sb == 2 && bwd_lds(FAM_SPLIT, net) > PINN_LDS_MAX) sb = 1;
  if (sb == 1 && bwd_lds(FAM_PIPE, net) > PINN_LDS_MAX) sb = 0;
  if (sf < 0 || sf > 2) sf = 0;
  if (sb < 0 || sb > 2) sb = 0;
  // The role-split sweeps do not spill layer 0 (its saved activations are one FMA pair and one tanh of the point: the
  // reverse sweep and dw_bf16 recompute them), so they only come as a pair, and with the bf16 dW kernel; a request for
  // one of them alone runs that sweep on schedule 1.
  const bool split_pair = sf == 2 && sb == 2 && net.prec_dw;
  if (!split_pair) { if (sf == 2) sf = 1; if (sb == 2) sb = 1; }
  // a sweep whose family lacks the plan's variant runs the 8-wave kernel (for a sine net that is both sweeps or neither:
  // without the pair no sweep is on schedule 2 here, so no plan mixes layouts)
  const unsigned variant = variant_bit(hbc.kind != 0, ptime, ff);
  if (sf == 1 && !(FAMILY_VARIANTS[FAM_PIPE] & variant)) sf = 0;
  if (sb == 1 && !(FAMILY_VARIANTS[FAM_PIPE] & variant)) sb = 0;
  // wide nets (hidden > 256), all three kernels in a bf16 mode, residual mode: the same 24-bit spill format
  const bool s24w_shape = HP > 256 && streams == 4 && net.prec_fwd && net.prec_bwd && net.prec_dw;
  // wide nets in the 24-bit format: the role-split sweeps at 64-column tiles where their LDS fits (hidden <= 448: the last
  // K region must fit twice in the 512-element image rows); $PINN_WSPLIT=0 keeps the 8-wave kernels.
  const bool wsplit = s24w_shape && L >= 2 && sw.wsplit != 0 && fwd_lds(FAM_WSPLIT, net) <= PINN_LDS_MAX &&
                      bwd_lds(FAM_WSPLIT, net) <= PINN_LDS_MAX;
  const bool s24w = s24w_shape && (!ff || wsplit);      // (the 8-wave FF kernels read and write SPILL_CLASSIC only)
  // The fused sweeps need the role-split pair on both sides, in one precision, and fit in LDS up to 7 hidden layers at hidden 256; deeper
  // nets keep the two launches.  $PINN_FUSE=0 keeps them too (same-build A/B).
  const bool fuse = sf == 2 && sb == 2 && split_pair && net.prec_fwd == net.prec_bwd && sw.fuse != 0 &&
                    fwdbwd_split_lds_bytes(HP, L) <= PINN_LDS_MAX;
  p->stagger = sw.stagger;
  if (sw.verbose)
    fprintf(stderr, "[pinn] plan: %ld pts, %d streams, HP %d, L %d, prec %d/%d/%d, wide %d, schedule fwd %d bwd %d\n",
            (long)n_points, streams, HP, L, net.prec_fwd, net.prec_bwd, net.prec_dw, (int)wide, sf, sb);
  if (sw.verbose && hbc.kind)
    fprintf(stderr, "[pinn] plan: hard wall conditions, lid-driven cavity at (%g, %g) x %g, lift power %d, lid sharpness %g\n",
            (double)hbc.x0, (double)hbc.y0, (double)hbc.inv_len, hbc.m, (double)hbc.r);
  const char* path = fuse ? "fused role-split kernel" : wsplit ? "wide role-split kernels" : sf == 2 ? "role-split kernels, two launches" : "8-wave kernels";
  if (sw.verbose && hbc.kind) fprintf(stderr, "[pinn] plan: constrained sweeps: %s (PINN_HBC_SPLIT=%d)\n", path, sw.hbc_split);
  if (sw.verbose && ptime) fprintf(stderr, "[pinn] plan: pseudo-time sweeps: %s (PINN_PTIME_SPLIT=%d)\n", path, sw.ptime_split);
  if (sw.verbose && ff && !keep_split)
    fprintf(stderr, "[pinn] plan: frozen sine first layer: 8-wave kernels, layer 0 stored (PINN_SCHED, PINN_WSPLIT, PINN_FUSE and PINN_S0_SKIP32 are not consulted)\n");
  if (sw.verbose && ff && keep_split) fprintf(stderr, "[pinn] plan: frozen sine sweeps: %s (PINN_FF_SPLIT=%d)\n", path, sw.ff_split);
  const Family fs = wsplit ? FAM_WSPLIT : sf == 2 ? FAM_SPLIT : sf == 1 ? FAM_PIPE : f8;
  const Family bs = wsplit ? FAM_WSPLIT : sb == 2 ? FAM_SPLIT : sb == 1 ? FAM_PIPE : b8;
  role(ROLE_FWD, f8, grid_f, lds_f, 0);
  role(ROLE_FWD_SAVE, fs, fs == f8 ? grid_f : grid_fp, fwd_lds(fs, net), 0);
  role(ROLE_BWD, bs, bs == b8 ? grid_b : grid_fp, bwd_lds(bs, net), 1);
  role(ROLE_FUSED, fuse ? FAM_FUSED : FAM_NONE, grid_fp, fuse ? fwdbwd_split_lds_bytes(HP, L) : 0, 0);
  if (L > 1) {
    int g = cus * bpc(lds_d) / (L - 1);
    if (g < 1) g = 1;
    if (g > p->ntiles) g = p->ntiles;
    p->groups = g;
  } else {
    p->groups = 0;
  }
  role(ROLE_DW, d8, p->groups, lds_d, 2);
  const int grid_part = p->role[ROLE_FWD].grid > p->role[ROLE_FWD_SAVE].grid ? p->role[ROLE_FWD].grid : p->role[ROLE_FWD_SAVE].grid;
  size_t off = 0;
  p->off_partials = off; off = align_up(off + (size_t)grid_part * PINN_NLOSS * 4, 256);
  p->off_oadj = off;     off = align_up(off + (size_t)4 * p->npad * 4, 256);
  p->bytes_fwd = off;
  p->off_sg = off;       off = align_up(off + (size_t)p->role[ROLE_BWD].grid * sg_total(HP, L) * 4, 256);
  p->off_slabs = off;    off = align_up(off + (size_t)(L - 1) * p->groups * HP * HP * 4, 256);
  // The spill layout (spill.h).  The role-split pair writes three 16-byte planes per register quad and no layer 0: its
  // S and Z-bar are sized for exactly that, (L - 1) blocks of 3/4 of the classic HP x 128 floats per tile (5.5 instead
  // of 8.9 GB each at 6x256 / 360 000 points).  Every other plan keeps [tile][L][HP x columns] blocks: an fp32 residual
  // plan without layer 0 in them ($PINN_S0_SKIP32=0 opts out), a wide all-bf16 residual plan in the 24-bit format.
  const size_t ablk = act_block(HP, wide ? 64 : PINN_TILE_COLS);
  const bool skip32 = streams == 4 && L >= 2 && !net.prec_fwd && !net.prec_bwd && !net.prec_dw && sw.s0_skip32 != 0 && !ff;
  p->spill = spill_make(split_pair ? SPILL_P24_COMPACT : s24w ? SPILL_P24_WIDE : skip32 ? SPILL_SKIP0 : SPILL_CLASSIC, ablk);
  for (int r = 0; r < ROLE_COUNT; ++r)
    if (p->role[r].family && !(FAMILY_VARIANTS[p->role[r].family] & variant)) {
      char what[96];
      snprintf(what, sizeof(what), "%s has no %s", p->role[r].name, variant_name(variant));
      return fail(-5, "pinn_plan_create: internal error: %s variant", what);
    }
  for (int r = 0; r < ROLE_COUNT; ++r)
    if (ROLE_SPILL_COL[r] >= 0 && p->role[r].family && (r != ROLE_DW || p->groups) &&
        !spill_is(p->spill, ablk, FAMILY_SPILLS[p->role[r].family][ROLE_SPILL_COL[r]]))
      return fail(-5, "pinn_plan_create: internal error: %s does not implement the plan's spill layout", p->role[r].name);
  const size_t spill_tile = spill_tile_floats(p->spill, L);
  // (+1 tile: the pipelined kernels work on PAIRS of tiles; an odd count's dummy partner spills into this scratch block)
  p->off_S = off;        off = align_up(off + (size_t)(p->ntiles + 1) * spill_tile * 4, 256);
  p->off_Zb = off;       off = align_up(off + (size_t)(p->ntiles + 1) * spill_tile * 4, 256);
  p->bytes_all = off;
  return 0;
}

// workspace carving (ws == null: the configure pass, which launches nothing)
static float* ws_at(void* ws, size_t off) { return ws ? reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + off) : nullptr; }
#define WS(p, off) ws_at(ws, (p)->off)

// The argument blocks, each filled in one place.  Each carries the plan's spill descriptor, and the residual-only
// (value-only) fields stay zero in value (residual) mode.
static FwdArgs fwd_args(const pinn_plan_s* plan, void* ws, const float* prep, const float* x, const float* y, int save, float scale) {
  FwdArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.n = (int)plan->n; a.ntiles = plan->ntiles; a.L = plan->net.L; a.n_out = plan->net.n_out;
  a.prep = prep; a.S = save ? WS(plan, off_S) : nullptr;
  a.scale = scale;
  a.partials = WS(plan, off_partials);
  a.spill = plan->spill;
  a.hbc = plan->hbc;
  a.ff = is_ff(plan->net);
  if (plan->streams == 4) {     // (these share their bytes with the value-mode fields)
    a.ptime = plan->ptime; a.anchor = plan->anchor; a.sigma = plan->sigma; a.sigma_p = plan->sigma_p;
  }
  return a;
}
static FwdArgs residual_fwd_args(const pinn_plan_s* plan, void* ws, const float* prep, const float* x, const float* y,
                                 const float* e, const float* w, float* vis_t_minus, float* vis_t_out, float* fields,
                                 float Re, float vis_t0, float alpha_evm, float coord_scale, int save, bool stagger) {
  FwdArgs a = fwd_args(plan, ws, prep, x, y, save, coord_scale);
  a.fld = fields; a.e = e; a.w = w; a.vtm = vis_t_minus; a.vis_used = vis_t_out;
  a.inv_re = 1.0f / Re; a.vis_t0 = vis_t0; a.alpha_evm = alpha_evm;
  a.nu_dev = plan->nu_dev; a.lap = plan->lap; a.cap_dev = plan->cap_dev;
  a.stagger = stagger && plan->ntiles > 4 * plan->role[ROLE_FWD].grid ? plan->stagger : 0;
  return a;
}
static BwdArgs bwd_args(const pinn_plan_s* plan, void* ws, const float* prep, const float* x, const float* y, float scale) {
  BwdArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.n = (int)plan->n; a.ntiles = plan->ntiles; a.L = plan->net.L; a.n_out = plan->net.n_out;
  a.prep = prep; a.S = WS(plan, off_S); a.Zb = WS(plan, off_Zb);
  a.scale = scale;
  a.sg = WS(plan, off_sg);
  a.spill = plan->spill;
  a.hbc = plan->hbc;
  a.ptime = plan->ptime; a.anchor = plan->anchor; a.sigma = plan->sigma; a.sigma_p = plan->sigma_p;
  a.ff = plan->streams == 4 && is_ff(plan->net);
  return a;
}
static BwdArgs residual_bwd_args(const pinn_plan_s* plan, void* ws, const float* prep, const float* x, const float* y,
                                 const float* e, const float* w, const float* vis_t, const float* fields,
                                 const float* coef_eq4, float Re, float coord_scale, float* ebar_out) {
  BwdArgs a = bwd_args(plan, ws, prep, x, y, coord_scale);
  a.fld = fields; a.e = e; a.w = w; a.vis_used = vis_t;
  for (int k = 0; k < 4; ++k) a.coef_eq[k] = coef_eq4[k];
  a.inv_re = 1.0f / Re; a.ebar = ebar_out;
  a.nu_dev = plan->nu_dev;
  return a;
}
static DwArgs dw_args(const pinn_plan_s* plan, void* ws, const float* prep, const float* x, const float* y) {
  DwArgs d;
  memset(&d, 0, sizeof(d));
  d.S = WS(plan, off_S); d.Zb = WS(plan, off_Zb);
  d.ntiles = plan->ntiles; d.L = plan->net.L; d.groups = plan->groups;
  d.slabs = WS(plan, off_slabs);
  d.x = x; d.y = y; d.prep = prep; d.n = (int)plan->n;
  d.spill = plan->spill;
  d.ff = plan->streams == 4 && is_ff(plan->net);
  return d;
}

// Raise the dynamic-LDS limit of every kernel the plan may launch, on the CURRENT device.
static int configure_plan(const pinn_plan_s* p) {
  FwdArgs fa = fwd_args(p, nullptr, nullptr, nullptr, nullptr, 0, 1.f);
  BwdArgs ba = bwd_args(p, nullptr, nullptr, nullptr, nullptr, 1.f);
  DwArgs da = dw_args(p, nullptr, nullptr, nullptr, nullptr);
  fa.configure = ba.configure = da.configure = 1;
  int rc = run_fwd(p, p->role[ROLE_FWD], fa, nullptr);
  if (!rc && p->role[ROLE_FWD_SAVE].family != p->role[ROLE_FWD].family) rc = run_fwd(p, p->role[ROLE_FWD_SAVE], fa, nullptr);
  if (!rc) rc = run_bwd(p, ba, nullptr);
  if (!rc && p->role[ROLE_FUSED].family) rc = run_fused(p, fa, ba, nullptr);
  if (!rc) rc = run_dw(p, da, nullptr);
  return rc;
}

extern "C" {

const char* pinn_last_error(void) { return g_err; }
int pinn_abi_version(void) { return 3; }   // 3: + pinn_plan_kernel; 2: + pinn_adam_step_dev, hidden <= 512 in every precision mode

int pinn_net_create(int n_out, int n_hidden_layers, int hidden, pinn_net_t* out) {
  if (!out) return fail(-22, "pinn_net_create: null out%s");
  if (n_out < 1 || n_out > 3) return fail(-22, "pinn_net_create: n_out must be 1..3%s");
  if (n_hidden_layers < 1 || n_hidden_layers > 64) return fail(-22, "pinn_net_create: hidden layers must be 1..64%s");
  if (hidden < 1 || hidden > PINN_MAX_HP) return fail(-22, "pinn_net_create: hidden width must be 1..512 (got %s%ld)", "", hidden);
  pinn_net_s* n = new (std::nothrow) pinn_net_s;
  if (!n) return fail(-12, "pinn_net_create: out of host memory%s");
  n->n_out = n_out; n->L = n_hidden_layers; n->H = hidden; n->HP = (hidden + 31) / 32 * 32;
  n->prec_fwd = n->prec_bwd = n->prec_dw = 0;
  n->wide = pick_wide(n);
  n->first_layer = PINN_FIRST_LAYER_TANH;
  n->shared = new (std::nothrow) NetShared;
  if (!n->shared) { delete n; return fail(-12, "pinn_net_create: out of host memory%s"); }
  n->shared->refs = 1; n->shared->first_layer = PINN_FIRST_LAYER_TANH;
  *out = n;
  return 0;
}
int pinn_net_set_first_layer(pinn_net_t net, int kind) {
  if (!net) return fail(-22, "pinn_net_set_first_layer: null net%s");
  if (kind != PINN_FIRST_LAYER_TANH && kind != PINN_FIRST_LAYER_SINE)
    return fail(-22, "pinn_net_set_first_layer: kind must be 0 (tanh) or 1 (frozen sine), got %s%ld", "", (long)kind);
  if (kind == PINN_FIRST_LAYER_SINE) {
    if (net->H % 2) return fail(-22, "pinn_net_set_first_layer: the frozen sine layer pairs a cosine with a sine row: the hidden width must be even (got %s%ld)", "", (long)net->H);
    if (net->L < 2)
      return fail(-22, "pinn_net_set_first_layer: the frozen sine layer needs at least 2 hidden layers (the output layer's gradient is formed from the last hidden layer by the tanh rule)%s");
  }
  net->first_layer = kind;
  net->shared->first_layer = kind;
  return 0;
}
int pinn_net_first_layer(pinn_net_t net) { return net ? net->first_layer : -1; }
int pinn_net_set_precision(pinn_net_t net, int prec_fwd, int prec_bwd, int prec_dw) {
  if (!net) return fail(-22, "pinn_net_set_precision: null net%s");
  if (prec_fwd < 0 || prec_fwd > 2 || prec_bwd < 0 || prec_bwd > 2 || prec_dw < 0 || prec_dw > 2)
    return fail(-22, "pinn_net_set_precision: precision must be 0 (fp32), 1 (bf16x3) or 2 (bf16)%s");
  // hidden > 256: fwd_bf16_wide / bwd_bf16_wide (64 features per wave) and the blocked dw_bf16_wide
  net->prec_fwd = prec_fwd; net->prec_bwd = prec_bwd; net->prec_dw = prec_dw;
  net->wide = pick_wide(net);
  return 0;
}
int pinn_net_destroy(pinn_net_t net) {
  if (net) shared_release(net->shared);
  delete net;
  return 0;
}
int64_t pinn_net_num_params(pinn_net_t net) { return net ? (int64_t)flat_total(net->H, net->L, net->n_out) : -1; }
int64_t pinn_net_prep_floats(pinn_net_t net) { return net ? (int64_t)prep_total(net->HP, net->L) : -1; }

int pinn_net_prepare(pinn_net_t net, const float* params, float* prep, void* stream) {
  if (!net || !params || !prep) return fail(-22, "pinn_net_prepare: null argument%s");
  int rc = launch_prep(params, prep, net->H, net->HP, net->L, net->n_out, net->prec_fwd, net->prec_bwd,
                       (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_net_prepare") : 0;
}

static int create_plan(pinn_net_t net, int64_t n_points, int streams, const HardBc& hbc, pinn_plan_t* out, bool ptime = false) {
  if (!net || !out) return fail(-22, "pinn_plan_create: null argument%s");
  if (streams != 1 && streams != 4) return fail(-22, "pinn_plan_create: streams must be 1 or 4%s");
  if (n_points < 1 || n_points > (int64_t)1 << 30) return fail(-22, "pinn_plan_create: bad point count %s%ld", "", (long)n_points);
  pinn_plan_s* p = new (std::nothrow) pinn_plan_s;
  if (!p) return fail(-12, "pinn_plan_create: out of host memory%s");
  int rc = resolve_plan(p, *net, (long)n_points, streams, num_cus(), read_switches(), hbc, ptime);
  if (rc) { delete p; return rc; }
  p->net.shared->refs.fetch_add(1);
  // The dynamic-LDS limit is per-device state of the HIP runtime and idempotent to raise; doing it here, per plan,
  // keeps the launch path free of cached "already configured" flags (no global mutable state; a process may drive
  // several devices and threads).
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) { ndev = 0; (void)hipGetLastError(); }
  if (ndev > 0) {     // (a host without a device can still size workspaces; it cannot launch anyway)
    rc = configure_plan(p);
    if (rc) { shared_release(p->net.shared); delete p; return hipfail(rc, "pinn_plan_create(kernel attributes)"); }
  }
  *out = p;
  return 0;
}
int pinn_plan_create(pinn_net_t net, int64_t n_points, int streams, pinn_plan_t* out) {
  return create_plan(net, n_points, streams, HardBc{}, out);
}
// the checked descriptor of pinn_plan_create_constrained / pinn_plan_create_pseudo_time (bc given, kind != 0)
static int hard_bc_of(pinn_net_t net, const pinn_hard_bc_t* bc, HardBc* h_out) {
  if (bc->kind != PINN_HARD_BC_CAVITY) return fail(-22, "pinn_plan_create_constrained: unknown kind %s%ld", "", (long)bc->kind);
  if (net->n_out != 3) return fail(-22, "pinn_plan_create_constrained: only a (u, v, p) net (n_out = 3) can be constrained%s");
  if (bc->lift_power < 1 || bc->lift_power > 8)
    return fail(-22, "pinn_plan_create_constrained: lift_power must be 1..8 (got %s%ld)", "", (long)bc->lift_power);
  if (!std::isfinite(bc->x0) || !std::isfinite(bc->y0) || !std::isfinite(bc->inv_len) || !std::isfinite(bc->lid_sharpness))
    return fail(-22, "pinn_plan_create_constrained: x0, y0, inv_len and lid_sharpness must be finite%s");
  if (!(bc->inv_len > 0.f)) return fail(-22, "pinn_plan_create_constrained: inv_len must be > 0%s");
  if (std::fabs(bc->lid_sharpness) > 150.f)      // exp(r / 2) must stay a finite float
    return fail(-22, "pinn_plan_create_constrained: |lid_sharpness| must be <= 150%s");
  HardBc h;
  h.kind = bc->kind; h.m = bc->lift_power; h.x0 = bc->x0; h.y0 = bc->y0; h.inv_len = bc->inv_len; h.r = bc->lid_sharpness;
  h.c = (float)(1.0 / std::cosh(0.5 * (double)bc->lid_sharpness));
  *h_out = h;
  return 0;
}
int pinn_plan_create_constrained(pinn_net_t net, int64_t n_points, int streams, const pinn_hard_bc_t* bc, pinn_plan_t* out) {
  if (!bc || bc->kind == PINN_HARD_BC_NONE) return pinn_plan_create(net, n_points, streams, out);
  if (!net || !out) return fail(-22, "pinn_plan_create_constrained: null argument%s");
  HardBc h;
  if (int rc = hard_bc_of(net, bc, &h)) return rc;
  return create_plan(net, n_points, streams, h, out);
}
int pinn_plan_create_pseudo_time(pinn_net_t net, int64_t n_points, const pinn_hard_bc_t* bc, pinn_plan_t* out) {
  if (!net || !out) return fail(-22, "pinn_plan_create_pseudo_time: null argument%s");
  if (net->n_out != 3) return fail(-22, "pinn_plan_create_pseudo_time: only a (u, v, p) net (n_out = 3) has a pseudo-time term%s");
  HardBc h{};
  if (bc && bc->kind != PINN_HARD_BC_NONE)
    if (int rc = hard_bc_of(net, bc, &h)) return rc;
  return create_plan(net, n_points, 4, h, out, true);
}
int pinn_plan_set_pseudo_time(pinn_plan_t plan, const float* anchor, float sigma, float sigma_p) {
  if (!plan) return fail(-22, "pinn_plan_set_pseudo_time: null plan%s");
  if (!plan->ptime) return fail(-22, "pinn_plan_set_pseudo_time: not a pseudo-time plan (pinn_plan_create_pseudo_time)%s");
  if (!std::isfinite(sigma) || !std::isfinite(sigma_p) || sigma < 0.f || sigma_p < 0.f)
    return fail(-22, "pinn_plan_set_pseudo_time: sigma and sigma_p must be finite and >= 0%s");
  if (!anchor) return fail(-22, "pinn_plan_set_pseudo_time: null anchor%s");
  if (reinterpret_cast<uintptr_t>(anchor) % 16 != 0) return fail(-22, "pinn_plan_set_pseudo_time: anchor must be 16-byte aligned%s");
  plan->anchor = anchor; plan->sigma = sigma; plan->sigma_p = sigma_p;
  return 0;
}
int pinn_plan_pseudo_time(pinn_plan_t plan, float* sigma, float* sigma_p) {
  if (!plan || !sigma || !sigma_p) return fail(-22, "pinn_plan_pseudo_time: null argument%s");
  if (!plan->ptime) return fail(-22, "pinn_plan_pseudo_time: not a pseudo-time plan (pinn_plan_create_pseudo_time)%s");
  *sigma = plan->sigma; *sigma_p = plan->sigma_p;
  return 0;
}
int pinn_plan_set_viscosity(pinn_plan_t plan, const float* nu_dev, float* lap) {
  if (!plan) return fail(-22, "pinn_plan_set_viscosity: null plan%s");
  if (plan->streams != 4) return fail(-22, "pinn_plan_set_viscosity: plan is not a residual (4-stream) plan%s");
  if (!nu_dev && lap) return fail(-22, "pinn_plan_set_viscosity: lap comes with nu_dev%s");
  if (reinterpret_cast<uintptr_t>(nu_dev) % 4 != 0) return fail(-22, "pinn_plan_set_viscosity: nu_dev must be 4-byte aligned%s");
  if (reinterpret_cast<uintptr_t>(lap) % 16 != 0) return fail(-22, "pinn_plan_set_viscosity: lap must be 16-byte aligned%s");
  plan->nu_dev = nu_dev; plan->lap = lap; plan->cap_dev = nullptr;
  return 0;
}
int pinn_plan_viscosity(pinn_plan_t plan, const float** nu_dev, float** lap) {
  if (!plan || !nu_dev || !lap) return fail(-22, "pinn_plan_viscosity: null argument%s");
  if (plan->streams != 4) return fail(-22, "pinn_plan_viscosity: plan is not a residual (4-stream) plan%s");
  *nu_dev = plan->nu_dev; *lap = plan->lap;
  return 0;
}
int pinn_plan_set_viscosity_cap(pinn_plan_t plan, const float* cap_dev) {
  if (!plan) return fail(-22, "pinn_plan_set_viscosity_cap: null plan%s");
  if (plan->streams != 4) return fail(-22, "pinn_plan_set_viscosity_cap: plan is not a residual (4-stream) plan%s");
  if (cap_dev && !plan->nu_dev) return fail(-22, "pinn_plan_set_viscosity_cap: cap_dev comes with nu_dev (pinn_plan_set_viscosity first)%s");
  if (reinterpret_cast<uintptr_t>(cap_dev) % 4 != 0) return fail(-22, "pinn_plan_set_viscosity_cap: cap_dev must be 4-byte aligned%s");
  plan->cap_dev = cap_dev;
  return 0;
}
int pinn_plan_viscosity_cap(pinn_plan_t plan, const float** cap_dev) {
  if (!plan || !cap_dev) return fail(-22, "pinn_plan_viscosity_cap: null argument%s");
  if (plan->streams != 4) return fail(-22, "pinn_plan_viscosity_cap: plan is not a residual (4-stream) plan%s");
  *cap_dev = plan->cap_dev;
  return 0;
}
int pinn_plan_hard_bc(pinn_plan_t plan, pinn_hard_bc_t* out) {
  if (!plan || !out) return fail(-22, "pinn_plan_hard_bc: null argument%s");
  const HardBc& h = plan->hbc;
  out->kind = h.kind; out->lift_power = h.m; out->x0 = h.x0; out->y0 = h.y0; out->inv_len = h.inv_len; out->lid_sharpness = h.r;
  return 0;
}
int pinn_plan_destroy(pinn_plan_t plan) {
  if (plan) shared_release(plan->net.shared);
  delete plan;
  return 0;
}
int64_t pinn_plan_padded_points(pinn_plan_t plan) { return plan ? plan->npad : -1; }
const char* pinn_plan_kernel(pinn_plan_t plan, int which) {
  if (!plan || which < 0 || which > 2) return nullptr;
  return plan->role[which == 0 ? ROLE_FWD_SAVE : which == 1 ? ROLE_BWD : ROLE_DW].name;
}
int64_t pinn_plan_workspace_bytes(pinn_plan_t plan, int with_backward) {
  if (!plan) return -1;
  return (int64_t)(with_backward ? plan->bytes_all : plan->bytes_fwd);
}

// A constrained plan takes the net's scaled derivatives for derivatives in the unit cavity's X, Y: the coordinate scale of
// the call must undo the plan's inv_len.
// A plan sees the first layer its net had when it was created; after pinn_net_set_first_layer changed the kind it
// would compute another function than the net's other plans, so every launch refuses it.
static int check_first_layer(const char* what, const pinn_plan_s* plan) {
  if (plan->net.shared->first_layer.load() != plan->net.first_layer)
    return fail(-22, "%s: the plan was created before the net's first-layer kind changed (pinn_net_set_first_layer): create it again", what);
  return 0;
}
static int check_hard_bc_scale(const char* what, const pinn_plan_s* plan, float coord_scale) {
  if (int rc = check_first_layer(what, plan)) return rc;
  if (plan->ptime && !plan->anchor)     // (every residual call comes through here)
    return fail(-22, "%s: the plan's pseudo-time anchors are unset (pinn_plan_set_pseudo_time)", what);
  if (plan->hbc.kind && !(std::fabs((double)coord_scale * (double)plan->hbc.inv_len - 1.0) <= 1e-6))
    return fail(-22, "%s: coord_scale x inv_len of the plan's hard wall conditions must be 1", what);
  return 0;
}

// the loss sums over the partials that a forward (or fused) launch of role `r` left, one row per workgroup
static int run_loss_sums(const Role& r, const FwdArgs& a, float* loss_sums, hipStream_t s, const char* what) {
  if (!loss_sums) return 0;
  int rc = launch_loss_sums(a.partials, r.grid, loss_sums, s);
  return rc ? hipfail(rc, what) : 0;
}

int pinn_residual_forward(pinn_plan_t plan, void* ws, const float* prep,
                          const float* x, const float* y, const float* e, const float* w,
                          float* vis_t_minus, float* vis_t_out, float* fields,
                          float Re, float vis_t0, float alpha_evm, float coord_scale,
                          int save, float* loss_sums, void* stream) {
  if (!plan || !ws || !prep || !x || !y || !fields) return fail(-22, "pinn_residual_forward: null argument%s");
  if (plan->streams != 4) return fail(-22, "pinn_residual_forward: plan is not a residual (4-stream) plan%s");
  if (!(Re > 0.f)) return fail(-22, "pinn_residual_forward: Re must be > 0%s");
  if (int rc = check_hard_bc_scale("pinn_residual_forward", plan, coord_scale)) return rc;
  const FwdArgs a = residual_fwd_args(plan, ws, prep, x, y, e, w, vis_t_minus, vis_t_out, fields, Re, vis_t0, alpha_evm,
                                      coord_scale, save, true);
  const Role& r = plan->role[save ? ROLE_FWD_SAVE : ROLE_FWD];
  int rc = run_fwd(plan, r, a, (hipStream_t)stream);
  if (rc) return hipfail(rc, "pinn_residual_forward");
  return run_loss_sums(r, a, loss_sums, (hipStream_t)stream, "pinn_residual_forward(loss sums)");
}

int pinn_residual_backward_phases(pinn_plan_t plan, void* ws, const float* prep,
                                  const float* x, const float* y, const float* e, const float* w,
                                  const float* vis_t, const float* fields, const float* coef_eq4,
                                  float Re, float coord_scale, float* ebar_out, int phases, void* stream) {
  if (!plan || !ws || !prep || !x || !y || !fields || !coef_eq4) return fail(-22, "pinn_residual_backward: null argument%s");
  if (plan->streams != 4) return fail(-22, "pinn_residual_backward: plan is not a residual (4-stream) plan%s");
  if (int rc = check_hard_bc_scale("pinn_residual_backward", plan, coord_scale)) return rc;
  const BwdArgs a = residual_bwd_args(plan, ws, prep, x, y, e, w, vis_t, fields, coef_eq4, Re, coord_scale, ebar_out);
  int rc = 0;
  if (phases & 1) {
    rc = run_bwd(plan, a, (hipStream_t)stream);
    if (rc) return hipfail(rc, "pinn_residual_backward");
  }
  if (phases & 2) rc = run_dw(plan, dw_args(plan, ws, prep, x, y), (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_residual_backward(dW)") : 0;
}

int pinn_residual_backward(pinn_plan_t plan, void* ws, const float* prep,
                           const float* x, const float* y, const float* e, const float* w,
                           const float* vis_t, const float* fields, const float* coef_eq4,
                           float Re, float coord_scale, float* ebar_out, void* stream) {
  return pinn_residual_backward_phases(plan, ws, prep, x, y, e, w, vis_t, fields, coef_eq4, Re, coord_scale,
                                       ebar_out, 3, stream);
}

int pinn_residual_forward_backward(pinn_plan_t plan, void* ws, const float* prep,
                                   const float* x, const float* y, const float* e, const float* w,
                                   float* vis_t_minus, float* vis_t_out, float* fields,
                                   const float* coef_eq4, float Re, float vis_t0, float alpha_evm,
                                   float coord_scale, float* loss_sums, float* ebar_out, void* stream) {
  if (!plan || !ws || !prep || !x || !y || !fields || !coef_eq4) return fail(-22, "pinn_residual_forward_backward: null argument%s");
  if (plan->streams != 4) return fail(-22, "pinn_residual_forward_backward: plan is not a residual (4-stream) plan%s");
  if (!plan->role[ROLE_FUSED].family) {
    int rc = pinn_residual_forward(plan, ws, prep, x, y, e, w, vis_t_minus, vis_t_out, fields, Re, vis_t0, alpha_evm,
                                   coord_scale, 1, loss_sums, stream);
    return rc ? rc : pinn_residual_backward(plan, ws, prep, x, y, e, w, vis_t_out, fields, coef_eq4, Re, coord_scale,
                                            ebar_out, stream);
  }
  if (!(Re > 0.f)) return fail(-22, "pinn_residual_forward_backward: Re must be > 0%s");
  if (int rc = check_hard_bc_scale("pinn_residual_forward_backward", plan, coord_scale)) return rc;
  // the argument blocks of the two launches it replaces (pinn_residual_forward, save = 1 / pinn_residual_backward),
  // except that the fused kernel never staggers its workgroups
  const FwdArgs fa = residual_fwd_args(plan, ws, prep, x, y, e, w, vis_t_minus, vis_t_out, fields, Re, vis_t0, alpha_evm,
                                       coord_scale, 1, false);
  const BwdArgs a = residual_bwd_args(plan, ws, prep, x, y, e, w, vis_t_out, fields, coef_eq4, Re, coord_scale, ebar_out);
  hipStream_t s = (hipStream_t)stream;
  int rc = run_fused(plan, fa, a, s);
  if (rc) return hipfail(rc, "pinn_residual_forward_backward");
  rc = run_loss_sums(plan->role[ROLE_FUSED], fa, loss_sums, s, "pinn_residual_forward_backward(loss sums)");
  if (rc) return rc;
  rc = run_dw(plan, dw_args(plan, ws, prep, x, y), s);
  return rc ? hipfail(rc, "pinn_residual_forward_backward(dW)") : 0;
}

int pinn_value_forward(pinn_plan_t plan, void* ws, const float* prep,
                       const float* x, const float* y,
                       float* const* pred3, const float* const* tgt3, const float* coef3,
                       int save, float* loss_sums, void* stream) {
  if (!plan || !ws || !prep || !x || !y) return fail(-22, "pinn_value_forward: null argument%s");
  if (plan->streams != 1) return fail(-22, "pinn_value_forward: plan is not a value (1-stream) plan%s");
  if (int rc = check_first_layer("pinn_value_forward", plan)) return rc;
  FwdArgs a = fwd_args(plan, ws, prep, x, y, save, 1.f);
  for (int c = 0; c < 3; ++c) {
    a.pred[c] = (pred3 && c < a.n_out) ? pred3[c] : nullptr;
    a.tgt[c] = (tgt3 && c < a.n_out) ? tgt3[c] : nullptr;
    a.coef[c] = coef3 ? coef3[c] : 0.f;
  }
  a.oadj = save ? WS(plan, off_oadj) : nullptr;
  const Role& r = plan->role[ROLE_FWD];
  int rc = run_fwd(plan, r, a, (hipStream_t)stream);
  if (rc) return hipfail(rc, "pinn_value_forward");
  return run_loss_sums(r, a, loss_sums, (hipStream_t)stream, "pinn_value_forward(loss sums)");
}

int pinn_value_backward(pinn_plan_t plan, void* ws, const float* prep,
                        const float* x, const float* y, const float* out_adj, void* stream) {
  if (!plan || !ws || !prep || !x || !y) return fail(-22, "pinn_value_backward: null argument%s");
  if (plan->streams != 1) return fail(-22, "pinn_value_backward: plan is not a value (1-stream) plan%s");
  if (int rc = check_first_layer("pinn_value_backward", plan)) return rc;
  BwdArgs a = bwd_args(plan, ws, prep, x, y, 1.f);
  a.oadj = out_adj ? out_adj : WS(plan, off_oadj);
  int rc = run_bwd(plan, a, (hipStream_t)stream);
  if (rc) return hipfail(rc, "pinn_value_backward");
  rc = run_dw(plan, dw_args(plan, ws, prep, x, y), (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_value_backward(dW)") : 0;
}

// the partial-sum sources of a gradient assembly: each plan's dW slabs and per-workgroup skinny accumulators
static int reduce_sources(const char* who, const pinn_net_s* net, int nsrc, const pinn_plan_t* plans, void* const* wss,
                          ReduceSrc* src) {
  for (int k = 0; k < nsrc; ++k) {
    pinn_plan_t p = plans[k];
    void* ws = wss[k];
    if (!p || !ws) return fail(-22, "%s: null plan/workspace", who);
    if (p->net.H != net->H || p->net.L != net->L || p->net.n_out != net->n_out)  // (precision may differ)
      return fail(-22, "%s: plan belongs to a different net", who);
    if (p->net.first_layer != net->first_layer)
      return fail(-22, "%s: the plan was created before the net's first-layer kind changed (pinn_net_set_first_layer): create it again", who);
    src[k].slabs = WS(p, off_slabs); src[k].groups = p->groups;
    src[k].sg = WS(p, off_sg); src[k].nwg = p->role[ROLE_BWD].grid;
  }
  return 0;
}

int pinn_grad_reduce(pinn_net_t net, int nsrc, const pinn_plan_t* plans, void* const* wss,
                     float* grads, int accumulate, void* stream) {
  if (!net || !plans || !wss || !grads) return fail(-22, "pinn_grad_reduce: null argument%s");
  if (nsrc < 1 || nsrc > 4) return fail(-22, "pinn_grad_reduce: nsrc must be 1..4%s");
  ReduceArgs r;
  memset(&r, 0, sizeof(r));
  r.nsrc = nsrc; r.H = net->H; r.HP = net->HP; r.L = net->L; r.n_out = net->n_out;
  r.grads = grads; r.accumulate = accumulate;
  r.frozen = is_ff(*net) ? 3 * net->H : 0;
  if (int rc = reduce_sources("pinn_grad_reduce", net, nsrc, plans, wss, r.src)) return rc;
  int rc = launch_reduce(r, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_grad_reduce") : 0;
}

int pinn_adam_step(float* params, const float* grads, float* m, float* v, int64_t n,
                   float lr, float beta1, float beta2, float eps, int64_t step, void* stream) {
  if (!params || !grads || !m || !v) return fail(-22, "pinn_adam_step: null argument%s");
  if (step < 1) return fail(-22, "pinn_adam_step: step must be >= 1%s");
  double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  int rc = launch_adam(params, grads, m, v, (long)n, (float)((double)lr / bc1), beta1, beta2, eps, (float)std::sqrt(bc2),
                       (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_adam_step") : 0;
}

int pinn_adam_step_dev(float* params, const float* grads, float* m, float* v, int64_t n,
                       float lr, float beta1, float beta2, float eps, int64_t* step_counter, void* stream) {
  if (!params || !grads || !m || !v || !step_counter) return fail(-22, "pinn_adam_step_dev: null argument%s");
  int rc = launch_adam_dev(params, grads, m, v, (long)n, lr, beta1, beta2, eps,
                           reinterpret_cast<long long*>(step_counter), (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_adam_step_dev") : 0;
}

int64_t pinn_resample_scratch_bytes(int64_t n_pool) {
  return n_pool < 1 || n_pool > (int64_t)1 << 30 ? -1 : (int64_t)resample_scratch_bytes((long)n_pool);
}

int pinn_resample_select(int64_t n_pool, const float* fields, int64_t npad, double w4, double k, double c,
                         double u, int64_t m, void* scratch, int64_t* out, void* stream) {
  if (!fields || !scratch || !out) return fail(-22, "pinn_resample_select: null argument%s");
  if (n_pool < 1 || n_pool > (int64_t)1 << 30) return fail(-22, "pinn_resample_select: pool size must be 1..2^30 (got %s%ld)", "", (long)n_pool);
  if (m < 1 || m > (int64_t)1 << 30) return fail(-22, "pinn_resample_select: m must be 1..2^30 (got %s%ld)", "", (long)m);
  if (npad < n_pool || npad % 4 != 0) return fail(-22, "pinn_resample_select: npad must be >= n_pool and a multiple of 4%s");
  if (reinterpret_cast<uintptr_t>(fields) % 16 != 0) return fail(-22, "pinn_resample_select: fields must be 16-byte aligned%s");
  if (!std::isfinite(k) || k < 0.0) return fail(-22, "pinn_resample_select: k must be finite and >= 0%s");
  if (!std::isfinite(c) || c < 0.0) return fail(-22, "pinn_resample_select: c must be finite and >= 0%s");
  if (!std::isfinite(w4) || w4 < 0.0) return fail(-22, "pinn_resample_select: w4 must be finite and >= 0%s");
  if (!(u >= 0.0 && u < 1.0)) return fail(-22, "pinn_resample_select: u must be in [0, 1)%s");
  int rc = launch_resample_select((long)n_pool, fields, (long)npad, w4, k, c, u, (long)m, scratch,
                                  reinterpret_cast<long long*>(out), (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_resample_select") : 0;
}

int pinn_resample_gather(const int64_t* idx, int64_t lo, int64_t hi, int64_t n_pool,
                         const float* src_x, const float* src_y, const float* src_w, const float* src_vtm,
                         float* dst_x, float* dst_y, float* dst_w, float* dst_vtm,
                         void* scratch, double* w_sum, void* stream) {
  if (!idx || !src_x || !src_y || !dst_x || !dst_y || !scratch) return fail(-22, "pinn_resample_gather: null argument%s");
  if (n_pool < 1 || n_pool > (int64_t)1 << 30) return fail(-22, "pinn_resample_gather: pool size must be 1..2^30 (got %s%ld)", "", (long)n_pool);
  if (lo < 0 || hi <= lo) return fail(-22, "pinn_resample_gather: need 0 <= lo < hi%s");
  if (!src_w != !dst_w) return fail(-22, "pinn_resample_gather: src_w and dst_w must both be given or both be NULL%s");
  if (!src_vtm != !dst_vtm) return fail(-22, "pinn_resample_gather: src_vtm and dst_vtm must both be given or both be NULL%s");
  if (w_sum && !dst_w) return fail(-22, "pinn_resample_gather: w_sum needs the weights%s");
  int rc = launch_resample_gather(reinterpret_cast<const long long*>(idx), (long)lo, (long)hi, (long)n_pool, src_x, src_y,
                                  src_w, src_vtm, dst_x, dst_y, dst_w, dst_vtm, scratch, w_sum, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_resample_gather") : 0;
}

int64_t pinn_lbfgs_workspace_bytes(int64_t n, int history) {
  if (n < 1 || n > (int64_t)1 << 30 || history < 1 || history > PINN_LBFGS_MAX_HISTORY) return -1;
  return (int64_t)lbfgs_workspace_bytes((long)n, (long)history);
}

static int lbfgs_args(const char* what, void* ws, int64_t n, int history) {
  if (!ws) return fail(-22, "%s: null workspace", what);
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "%s: n must be 1..2^30", what);
  if (history < 1 || history > PINN_LBFGS_MAX_HISTORY) return fail(-22, "%s: history must be 1..1024", what);
  if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return fail(-22, "%s: workspace must be 256-byte aligned", what);
  return 0;
}

int pinn_lbfgs_reset(void* ws, int64_t n, int history, void* stream) {
  if (int rc = lbfgs_args("pinn_lbfgs_reset", ws, n, history)) return rc;
  int rc = launch_lbfgs_reset(ws, (long)n, history, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_lbfgs_reset") : 0;
}

int pinn_lbfgs_direction(void* ws, int64_t n, int history, const float* g, float t_prev, float* d, double* result,
                         void* stream) {
  if (int rc = lbfgs_args("pinn_lbfgs_direction", ws, n, history)) return rc;
  if (!g || !d || !result) return fail(-22, "pinn_lbfgs_direction: null argument%s");
  if (reinterpret_cast<uintptr_t>(g) % 16 != 0 || reinterpret_cast<uintptr_t>(d) % 16 != 0)
    return fail(-22, "pinn_lbfgs_direction: g and d must be 16-byte aligned%s");
  if (!std::isfinite(t_prev)) return fail(-22, "pinn_lbfgs_direction: t_prev must be finite%s");
  int rc = launch_lbfgs_direction(ws, (long)n, history, g, t_prev, d, result, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_lbfgs_direction") : 0;
}

int pinn_lbfgs_probe(void* ws, int64_t n, int history, const float* g, const float* d, double* result, void* stream) {
  if (int rc = lbfgs_args("pinn_lbfgs_probe", ws, n, history)) return rc;
  if (!g || !d || !result) return fail(-22, "pinn_lbfgs_probe: null argument%s");
  if (reinterpret_cast<uintptr_t>(g) % 16 != 0 || reinterpret_cast<uintptr_t>(d) % 16 != 0)
    return fail(-22, "pinn_lbfgs_probe: g and d must be 16-byte aligned%s");
  int rc = launch_lbfgs_probe(ws, (long)n, history, g, d, result, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_lbfgs_probe") : 0;
}

int64_t pinn_balance_partials_count(int64_t n) {
  return n < 1 || n > (int64_t)1 << 30 ? -1 : (int64_t)balance_blocks((long)n) * 6;
}

static int reduce_terms(const char* what, pinn_net_t net, const int* nsrc3, const pinn_plan_t* plans, void* const* wss,
                        float* const* out3, int accumulate_mask, double* partials, double* gram, void* stream) {
  if (!net || !nsrc3 || !out3) return fail(-22, "%s: null argument", what);
  TermReduceArgs r;
  memset(&r, 0, sizeof(r));
  int total = 0;
  for (int t = 0; t < 3; ++t) {
    if (nsrc3[t] < 0) return fail(-22, "%s: negative source count", what);
    if (nsrc3[t] > 0 && !out3[t]) return fail(-22, "%s: a group with sources needs its output", what);
    r.nsrc[t] = nsrc3[t]; r.out[t] = out3[t];
    total += nsrc3[t];
  }
  if (total < 1 || total > 4) return fail(-22, "%s: 1..4 sources in all", what);
  if (!plans || !wss) return fail(-22, "%s: null argument", what);
  r.H = net->H; r.HP = net->HP; r.L = net->L; r.n_out = net->n_out;
  r.acc_mask = accumulate_mask & 7; r.partials = partials; r.gram = gram;
  r.frozen = is_ff(*net) ? 3 * net->H : 0;
  if (int rc = reduce_sources(what, net, total, plans, wss, r.src)) return rc;
  int rc = launch_reduce_terms(r, (hipStream_t)stream);
  return rc ? hipfail(rc, what) : 0;
}

int pinn_grad_reduce_terms(pinn_net_t net, const int* nsrc3, const pinn_plan_t* plans, void* const* wss,
                           float* const* out3, int accumulate_mask, double* partials, void* stream) {
  return reduce_terms("pinn_grad_reduce_terms", net, nsrc3, plans, wss, out3, accumulate_mask, partials, nullptr, stream);
}

int pinn_grad_reduce_terms_gram(pinn_net_t net, const int* nsrc3, const pinn_plan_t* plans, void* const* wss,
                                float* const* out3, int accumulate_mask, double* partials, double* gram_partials,
                                void* stream) {
  return reduce_terms("pinn_grad_reduce_terms_gram", net, nsrc3, plans, wss, out3, accumulate_mask, partials,
                      gram_partials, stream);
}

int pinn_balance_stats(const float* const* vec3, int64_t n, double* partials, void* stream) {
  if (!vec3 || !partials) return fail(-22, "pinn_balance_stats: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_balance_stats: n must be 1..2^30%s");
  int rc = launch_balance_stats(vec3[0], vec3[1], vec3[2], (long)n, partials, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_balance_stats") : 0;
}

int pinn_balance_update(const double* partials, int64_t n, int terms, double beta, float* lam, double* record,
                        void* stream) {
  if (!partials || !lam || !record) return fail(-22, "pinn_balance_update: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_balance_update: n must be 1..2^30%s");
  if (terms < 0 || terms > 3) return fail(-22, "pinn_balance_update: terms must be 0..3%s");
  if (!(beta > 0.0 && beta <= 1.0)) return fail(-22, "pinn_balance_update: beta must be in (0, 1]%s");
  int rc = launch_balance_update(partials, (long)n, terms, beta, lam, record, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_balance_update") : 0;
}

int pinn_balance_combine(float* g, const float* gr, const float* gb, const float* gs, const float* lam, int64_t n,
                         void* stream) {
  if (!g || !gr || !gb || !lam) return fail(-22, "pinn_balance_combine: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_balance_combine: n must be 1..2^30%s");
  int rc = launch_balance_combine(g, gr, gb, gs, lam, (long)n, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_balance_combine") : 0;
}

int64_t pinn_confgrad_partials_count(int64_t n) { return pinn_balance_partials_count(n); }

int pinn_confgrad_gram(const float* const* vec3, int64_t n, double* partials, void* stream) {
  if (!vec3 || !partials) return fail(-22, "pinn_confgrad_gram: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_confgrad_gram: n must be 1..2^30%s");
  int rc = launch_confgrad_gram(vec3[0], vec3[1], vec3[2], (long)n, partials, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_confgrad_gram") : 0;
}

int pinn_confgrad_coef(const double* partials, int64_t n, int nterms, float* coef, double* record, void* stream) {
  if (!partials || !coef || !record) return fail(-22, "pinn_confgrad_coef: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_confgrad_coef: n must be 1..2^30%s");
  if (nterms < 2 || nterms > 3) return fail(-22, "pinn_confgrad_coef: nterms must be 2 or 3%s");
  int rc = launch_confgrad_coef(partials, (long)n, nterms, coef, record, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_confgrad_coef") : 0;
}

int pinn_confgrad_combine(float* g, const float* gr, const float* gb, const float* gs, const float* coef, int64_t n,
                          void* stream) {
  if (!g || !gr || !gb || !coef) return fail(-22, "pinn_confgrad_combine: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_confgrad_combine: n must be 1..2^30%s");
  int rc = launch_confgrad_combine(g, gr, gb, gs, coef, (long)n, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_confgrad_combine") : 0;
}

int pinn_batch_draw(int64_t n, int64_t b, uint64_t seed, int rank, int64_t* counter,
                    const float* src_x, const float* src_y, const float* src_w, const float* src_vtm,
                    float* dst_x, float* dst_y, float* dst_w, float* dst_vtm, int64_t* idx, void* stream) {
  if (!counter || !src_x || !src_y || !dst_x || !dst_y || !idx) return fail(-22, "pinn_batch_draw: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_batch_draw: store size must be 1..2^30 (got %s%ld)", "", (long)n);
  if (b < 1 || b > n) return fail(-22, "pinn_batch_draw: batch size must be 1..n (got %s%ld)", "", (long)b);
  if (rank < 0) return fail(-22, "pinn_batch_draw: rank must be >= 0%s");
  if (!src_w != !dst_w) return fail(-22, "pinn_batch_draw: src_w and dst_w must both be given or both be NULL%s");
  if (!src_vtm != !dst_vtm) return fail(-22, "pinn_batch_draw: src_vtm and dst_vtm must both be given or both be NULL%s");
  BatchDrawArgs a;
  a.n = (long)n; a.b = (long)b;
  a.seed = (unsigned)(seed & 0xffffffffu); a.rank = (unsigned)rank;
  a.counter = reinterpret_cast<long long*>(counter);
  a.sx = src_x; a.sy = src_y; a.sw = src_w; a.sv = src_vtm;
  a.dx = dst_x; a.dy = dst_y; a.dw = dst_w; a.dv = dst_vtm;
  a.idx = reinterpret_cast<long long*>(idx);
  int rc = launch_batch_draw(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_batch_draw") : 0;
}

int pinn_batch_scatter(const int64_t* idx, int64_t b, int64_t n, const float* batch_vtm, float* store_vtm,
                       void* stream) {
  if (!idx || !batch_vtm || !store_vtm) return fail(-22, "pinn_batch_scatter: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_batch_scatter: store size must be 1..2^30 (got %s%ld)", "", (long)n);
  if (b < 1 || b > n) return fail(-22, "pinn_batch_scatter: batch size must be 1..n (got %s%ld)", "", (long)b);
  int rc = launch_batch_scatter(reinterpret_cast<const long long*>(idx), (long)b, (long)n, batch_vtm, store_vtm,
                                (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_batch_scatter") : 0;
}

int64_t pinn_rba_scratch_bytes(int64_t n) {
  return n < 1 || n > (int64_t)1 << 30 ? -1 : (int64_t)rba_scratch_bytes((long)n);
}

static int rba_planes(const char* what, int64_t n, const float* fields, int64_t npad, double w4) {
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "%s: n must be 1..2^30 (got %ld)", what, (long)n);
  if (!fields) return fail(-22, "%s: null field planes", what);
  if (npad < n || npad % 4 != 0) return fail(-22, "%s: npad must be >= n and a multiple of 4", what);
  if (reinterpret_cast<uintptr_t>(fields) % 16 != 0) return fail(-22, "%s: fields must be 16-byte aligned", what);
  if (!std::isfinite(w4) || w4 < 0.0) return fail(-22, "%s: w4 must be finite and >= 0", what);
  return 0;
}

int pinn_rba_stats(int64_t n, const float* fields, int64_t npad, double w4, double* scratch, void* stream) {
  if (int rc = rba_planes("pinn_rba_stats", n, fields, npad, w4)) return rc;
  if (!scratch || reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return fail(-22, "pinn_rba_stats: scratch must be given and 8-byte aligned%s");
  int rc = launch_rba_stats((long)n, fields, (long)npad, w4, scratch, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_rba_stats") : 0;
}

int pinn_rba_apply(int64_t n, const float* fields, int64_t npad, double w4, double gamma, double eta,
                   const int64_t* idx, int64_t n_store, const float* s, float* lam, float* w, double* scratch,
                   double* record, void* stream) {
  if (int rc = rba_planes("pinn_rba_apply", n, fields, npad, w4)) return rc;
  if (!lam || !w || !scratch || !record) return fail(-22, "pinn_rba_apply: null argument%s");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return fail(-22, "pinn_rba_apply: scratch must be 8-byte aligned%s");
  if (n_store < 1 || n_store > (int64_t)1 << 30) return fail(-22, "pinn_rba_apply: store size must be 1..2^30 (got %s%ld)", "", (long)n_store);
  if (!idx && n > n_store) return fail(-22, "pinn_rba_apply: without idx n must be <= n_store%s");
  if (!(gamma > 0.0 && gamma <= 1.0)) return fail(-22, "pinn_rba_apply: gamma must be in (0, 1]%s");
  if (!std::isfinite(eta) || eta < 0.0) return fail(-22, "pinn_rba_apply: eta must be finite and >= 0%s");
  if (reinterpret_cast<uintptr_t>(lam) % 16 != 0 || reinterpret_cast<uintptr_t>(w) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(s) % 16 != 0)
    return fail(-22, "pinn_rba_apply: s, lam and w must be 16-byte aligned%s");
  if (lam == w || s == lam || s == w) return fail(-22, "pinn_rba_apply: s, lam and w must be distinct buffers%s");
  RbaApplyArgs a;
  a.n = (long)n; a.npad = (long)npad; a.n_store = (long)n_store;
  a.fld = fields; a.w4 = w4; a.gamma = gamma; a.eta = eta;
  a.idx = reinterpret_cast<const long long*>(idx);
  a.s = s; a.lam = lam; a.w = w; a.scratch = scratch; a.record = record;
  int rc = launch_rba_apply(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_rba_apply") : 0;
}

int pinn_rba_fill(int64_t n, double init, const float* s, float* lam, float* w, void* stream) {
  if (!lam || !w) return fail(-22, "pinn_rba_fill: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_rba_fill: n must be 1..2^30 (got %s%ld)", "", (long)n);
  if (!std::isfinite(init) || init < 0.0) return fail(-22, "pinn_rba_fill: init must be finite and >= 0%s");
  int rc = launch_rba_fill((long)n, init, s, lam, w, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_rba_fill") : 0;
}

// ---------------------------------------------------------------------------
// learning-rate schedules and gradient clipping for Adam (optim.hip)
// ---------------------------------------------------------------------------
static int check_schedule(const char* what, const pinn_lr_schedule_t* s) {
  if (!s) return fail(-22, "%s: null schedule", what);
  if (s->kind < PINN_LR_CONSTANT || s->kind > PINN_LR_COSINE) return fail(-22, "%s: unknown schedule kind %ld", what, (long)s->kind);
  if (s->warmup_epochs < 0) return fail(-22, "%s: warmup_epochs must be >= 0", what);
  if (s->warmup_epochs > 0 && !(s->warmup_start >= 0.0 && s->warmup_start <= 1.0))
    return fail(-22, "%s: warmup_start must be in [0, 1]", what);
  if (s->kind == PINN_LR_CONSTANT) return 0;
  if (s->kind == PINN_LR_COSINE) {
    if (s->t_max < 1) return fail(-22, "%s: t_max must be >= 1", what);
    if (!std::isfinite(s->eta_min)) return fail(-22, "%s: eta_min must be finite", what);
    return 0;
  }
  if (!(s->gamma > 0.0) || !std::isfinite(s->gamma)) return fail(-22, "%s: gamma must be finite and > 0", what);
  if (s->kind == PINN_LR_STEP && s->step_size < 1) return fail(-22, "%s: step_size must be >= 1", what);
  if (s->kind == PINN_LR_MULTISTEP) {
    if (s->n_milestones < 0 || s->n_milestones > PINN_LR_MAX_MILESTONES)
      return fail(-22, "%s: at most 16 milestones (got %ld)", what, (long)s->n_milestones);
    for (int i = 0; i < s->n_milestones; ++i)
      if (s->milestones[i] < 0 || (i > 0 && s->milestones[i] < s->milestones[i - 1]))
        return fail(-22, "%s: milestones must be >= 0 and non-decreasing", what);
  }
  return 0;
}

double pinn_lr_schedule_value(const pinn_lr_schedule_t* schedule, double lr0, int64_t e) {
  if (check_schedule("pinn_lr_schedule_value", schedule)) return NAN;
  if (e < 0) { fail(-22, "pinn_lr_schedule_value: e must be >= 0%s"); return NAN; }
  return lr_schedule_value(*schedule, lr0, (long long)e);
}

int64_t pinn_grad_sqnorm_scratch_bytes(void) { return (int64_t)grad_sqnorm_scratch_bytes(); }

int pinn_grad_sqnorm(const float* g0, int64_t n0, const float* g1, int64_t n1, double* scratch, void* stream) {
  if (!g0 || !scratch) return fail(-22, "pinn_grad_sqnorm: null argument%s");
  if (n0 < 1 || n0 > (int64_t)1 << 30) return fail(-22, "pinn_grad_sqnorm: n0 must be 1..2^30 (got %s%ld)", "", (long)n0);
  if (n1 < 0 || n1 > (int64_t)1 << 30) return fail(-22, "pinn_grad_sqnorm: n1 must be 0..2^30 (got %s%ld)", "", (long)n1);
  if ((n1 > 0) != (g1 != nullptr)) return fail(-22, "pinn_grad_sqnorm: g1 must be given exactly when n1 > 0%s");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return fail(-22, "pinn_grad_sqnorm: scratch must be 8-byte aligned%s");
  if (reinterpret_cast<uintptr_t>(g0) % 4 != 0 || reinterpret_cast<uintptr_t>(g1) % 4 != 0)
    return fail(-22, "pinn_grad_sqnorm: the vectors must be 4-byte aligned%s");
  int rc = launch_grad_sqnorm(g0, (long)n0, g1, (long)n1, scratch, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_grad_sqnorm") : 0;
}

int pinn_adam_step_sched(float* params, const float* grads, float* m, float* v, int64_t n,
                         const pinn_lr_schedule_t* schedule, double lr0, float beta1, float beta2, float eps,
                         int64_t* step_counter, int64_t* epoch, int advance, const double* sqnorm, double max_norm,
                         double* record, void* stream) {
  if (!params || !grads || !m || !v || !step_counter || !epoch || !record)
    return fail(-22, "pinn_adam_step_sched: null argument%s");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_adam_step_sched: n must be 1..2^30 (got %s%ld)", "", (long)n);
  if (int rc = check_schedule("pinn_adam_step_sched", schedule)) return rc;
  if (!std::isfinite(lr0)) return fail(-22, "pinn_adam_step_sched: lr0 must be finite%s");
  if (sqnorm && !(max_norm > 0.0)) return fail(-22, "pinn_adam_step_sched: max_norm must be > 0 when sqnorm is given%s");
  if (reinterpret_cast<uintptr_t>(sqnorm) % 8 != 0 || reinterpret_cast<uintptr_t>(record) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(epoch) % 8 != 0)
    return fail(-22, "pinn_adam_step_sched: epoch, sqnorm and record must be 8-byte aligned%s");
  AdamSchedArgs a;
  a.p = params; a.g = grads; a.m = m; a.v = v; a.n = (long)n;
  a.sched = *schedule; a.lr0 = lr0; a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  a.step_counter = reinterpret_cast<long long*>(step_counter);
  a.epoch = reinterpret_cast<long long*>(epoch);
  a.advance = advance != 0; a.sq = sqnorm; a.max_norm = max_norm; a.record = record;
  int rc = launch_adam_sched(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_adam_step_sched") : 0;
}

// ---------------------------------------------------------------------------
// random weight factorization of the dense layers (rwf.hip)
// ---------------------------------------------------------------------------
static RwfNet rwf_net(const pinn_net_s* net) {
  RwfNet n;
  n.H = net->H; n.L = net->L; n.n_out = net->n_out;
  return n;
}
static bool misaligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 != 0; }
// [a, a + na) and [b, b + nb) floats share an entry
static bool overlap(const float* a, size_t na, const float* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + 4 * nb && b0 < a0 + 4 * na;
}

int64_t pinn_rwf_rows(pinn_net_t net) { return net ? (int64_t)rwf_rows(rwf_net(net)) : -1; }

int pinn_rwf_split(pinn_net_t net, const float* params, const float* s, float* theta, void* stream) {
  if (!net || !params || !s || !theta) return fail(-22, "pinn_rwf_split: null argument%s");
  if (misaligned4(params) || misaligned4(s) || misaligned4(theta))
    return fail(-22, "pinn_rwf_split: the vectors must be 4-byte aligned%s");
  const RwfNet n = rwf_net(net);
  const size_t P = flat_total(n.H, n.L, n.n_out), R = (size_t)rwf_rows(n);
  if (overlap(theta, P + R, params, P) || overlap(theta, P + R, s, R))
    return fail(-22, "pinn_rwf_split: theta must not overlap params or s%s");
  int rc = launch_rwf_split(n, params, s, theta, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_rwf_split") : 0;
}

int pinn_rwf_compose(pinn_net_t net, const float* theta, float* params, void* stream) {
  if (!net || !theta || !params) return fail(-22, "pinn_rwf_compose: null argument%s");
  if (misaligned4(theta) || misaligned4(params)) return fail(-22, "pinn_rwf_compose: the vectors must be 4-byte aligned%s");
  const RwfNet n = rwf_net(net);
  const size_t P = flat_total(n.H, n.L, n.n_out), R = (size_t)rwf_rows(n);
  if (overlap(theta, P + R, params, P)) return fail(-22, "pinn_rwf_compose: params must not overlap theta%s");
  int rc = launch_rwf_compose(n, theta, params, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_rwf_compose") : 0;
}

int pinn_rwf_grad(pinn_net_t net, const float* theta, const float* grads, float* gtheta, void* stream) {
  if (!net || !theta || !grads || !gtheta) return fail(-22, "pinn_rwf_grad: null argument%s");
  if (misaligned4(theta) || misaligned4(grads) || misaligned4(gtheta))
    return fail(-22, "pinn_rwf_grad: the vectors must be 4-byte aligned%s");
  const RwfNet n = rwf_net(net);
  const size_t P = flat_total(n.H, n.L, n.n_out), R = (size_t)rwf_rows(n);
  if (overlap(gtheta, P + R, theta, P + R) || overlap(gtheta, P + R, grads, P))
    return fail(-22, "pinn_rwf_grad: gtheta must not overlap theta or grads%s");
  int rc = launch_rwf_grad(n, theta, grads, gtheta, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_rwf_grad") : 0;
}

int64_t pinn_ptime_scratch_bytes(int64_t n) {
  return n < 1 || n > (int64_t)1 << 30 ? -1 : (int64_t)ptime_scratch_bytes((long)n);
}

int pinn_ptime_advance(int64_t n, const float* fields, int64_t npad, const float* w, float* anchor, int64_t every,
                       int force, double* scratch, double* record, void* stream) {
  static_assert(PINN_PTIME_RECORD == PTIME_RECORD, "pseudo-time record size mismatch");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_ptime_advance: n must be 1..2^30 (got %s%ld)", "", (long)n);
  if (!fields || !anchor || !scratch || !record) return fail(-22, "pinn_ptime_advance: null argument%s");
  if (npad < n || npad % 4 != 0) return fail(-22, "pinn_ptime_advance: npad must be >= n and a multiple of 4%s");
  if (every < 0) return fail(-22, "pinn_ptime_advance: every must be >= 0 (got %s%ld)", "", (long)every);
  if (reinterpret_cast<uintptr_t>(fields) % 16 != 0 || reinterpret_cast<uintptr_t>(anchor) % 16 != 0 ||
      reinterpret_cast<uintptr_t>(w) % 16 != 0)
    return fail(-22, "pinn_ptime_advance: fields, anchor and w must be 16-byte aligned%s");
  if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0 || reinterpret_cast<uintptr_t>(record) % 8 != 0)
    return fail(-22, "pinn_ptime_advance: scratch and record must be 8-byte aligned%s");
  PtimeArgs a;
  a.n = (long)n; a.npad = (long)npad; a.fld = fields; a.w = w; a.anchor = anchor;
  a.every = (double)every; a.force = force != 0; a.scratch = scratch; a.record = record;
  int rc = launch_ptime_advance(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_ptime_advance") : 0;
}

int64_t pinn_val_scratch_bytes(void) { return (int64_t)val_scratch_bytes(); }

static bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }

int pinn_val_stats(int64_t n, const float* const* pred3, const float* const* tgt3, int metric, double t, int64_t every,
                   double* scratch, double* state, double* ring, int64_t capacity, void* stream) {
  static_assert(PINN_VAL_RECORD == VAL_RECORD && PINN_VAL_STATE == VAL_STATE, "validation record / state size mismatch");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_val_stats: n must be 1..2^30 (got %s%ld)", "", (long)n);
  if (capacity < 1 || capacity > (int64_t)1 << 30) return fail(-22, "pinn_val_stats: capacity must be 1..2^30 (got %s%ld)", "", (long)capacity);
  if (every < 1) return fail(-22, "pinn_val_stats: every must be >= 1 (got %s%ld)", "", (long)every);
  if (metric < 0 || metric > 4) return fail(-22, "pinn_val_stats: metric must be 0..4 (got %s%ld)", "", (long)metric);
  if (!(t == -1.0 || (t >= 0.0 && std::isfinite(t)))) return fail(-22, "pinn_val_stats: t must be -1 (the cadence) or finite and >= 0%s");
  if (!pred3 || !tgt3 || !scratch || !state || !ring) return fail(-22, "pinn_val_stats: null argument%s");
  if (misaligned(scratch, 8) || misaligned(state, 8) || misaligned(ring, 8))
    return fail(-22, "pinn_val_stats: scratch, state and ring must be 8-byte aligned%s");
  ValStatsArgs a;
  for (int c = 0; c < 3; ++c) {
    a.pred[c] = pred3[c]; a.tgt[c] = tgt3[c];
    if (c < 2 && (!a.pred[c] || !a.tgt[c])) return fail(-22, "pinn_val_stats: the u and v planes must be given%s");
    if (misaligned(a.pred[c], 16) || misaligned(a.tgt[c], 16)) return fail(-22, "pinn_val_stats: every plane must be 16-byte aligned%s");
  }
  if (!a.pred[2] != !a.tgt[2]) return fail(-22, "pinn_val_stats: the pressure prediction and target come together%s");
  if (metric >= 3 && !a.pred[2]) return fail(-22, "pinn_val_stats: a pressure metric needs the pressure planes%s");
  a.n = (long)n; a.capacity = (long)capacity; a.metric = metric; a.t = t; a.every = (double)every;
  a.scratch = scratch; a.state = state; a.ring = ring;
  int rc = launch_val_stats(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_val_stats") : 0;
}

int pinn_val_keep(const float* src0, float* dst0, int64_t n0, const float* src1, float* dst1, int64_t n1,
                  const double* state, void* stream) {
  if (!src0 || !dst0 || !state) return fail(-22, "pinn_val_keep: null argument%s");
  if (n0 < 1 || n0 > (int64_t)1 << 30) return fail(-22, "pinn_val_keep: n0 must be 1..2^30 (got %s%ld)", "", (long)n0);
  if (n1 < 0 || n1 > (int64_t)1 << 30) return fail(-22, "pinn_val_keep: n1 must be 0..2^30 (got %s%ld)", "", (long)n1);
  if (n1 > 0 && (!src1 || !dst1)) return fail(-22, "pinn_val_keep: the second segment has a length but no buffers%s");
  if (misaligned(src0, 4) || misaligned(dst0, 4) || misaligned(src1, 4) || misaligned(dst1, 4) || misaligned(state, 8))
    return fail(-22, "pinn_val_keep: the segments must be 4-byte aligned, state 8-byte%s");
  ValKeepArgs a;
  a.src[0] = src0; a.dst[0] = dst0; a.n[0] = (long)n0;
  a.src[1] = n1 > 0 ? src1 : nullptr; a.dst[1] = n1 > 0 ? dst1 : nullptr; a.n[1] = (long)n1;
  a.state = state;
  int rc = launch_val_keep(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_val_keep") : 0;
}

// ---- flow diagnostics (flowdiag.hip) ----
int64_t pinn_flow_scratch_bytes(void) { return (int64_t)flow_scratch_bytes(); }

static int flow_grid(const char* what, int64_t nx, int64_t ny, const float* fields, int64_t npad) {
  if (nx < 3 || nx > (int64_t)1 << 30) return fail(-22, "%s: nx must be 3..2^30 (got %ld)", what, (long)nx);
  if (ny < 3 || ny > (int64_t)1 << 30) return fail(-22, "%s: ny must be 3..2^30 (got %ld)", what, (long)ny);
  if (nx * ny > (int64_t)1 << 30) return fail(-22, "%s: nx * ny must be at most 2^30 (got %ld)", what, (long)(nx * ny));
  if (npad < nx * ny || npad % 4 != 0) return fail(-22, "%s: npad must be a multiple of 4 and >= nx * ny (got %ld)", what, (long)npad);
  if (!fields || misaligned(fields, 16)) return fail(-22, "%s: fields must be given and 16-byte aligned", what);
  return 0;
}

int pinn_flow_stream_function(int64_t nx, int64_t ny, const float* fields, int64_t npad, const double* ys, double* psi,
                              void* stream) {
  if (int rc = flow_grid("pinn_flow_stream_function", nx, ny, fields, npad)) return rc;
  if (!ys || !psi) return fail(-22, "pinn_flow_stream_function: null argument%s");
  if (misaligned(ys, 8) || misaligned(psi, 16)) return fail(-22, "pinn_flow_stream_function: ys must be 8-byte aligned, psi 16-byte%s");
  FlowPsiArgs a;
  a.nx = (long)nx; a.ny = (long)ny; a.npad = (long)npad; a.fld = fields; a.ys = ys; a.psi = psi;
  int rc = launch_flow_psi(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_flow_stream_function") : 0;
}

int pinn_flow_stats(int64_t nx, int64_t ny, const float* fields, int64_t npad, const double* xs, const double* ys,
                    const double* psi, double eps, double t, int64_t every, double* scratch, double* state, double* ring,
                    int64_t capacity, void* stream) {
  static_assert(PINN_FLOW_RECORD == FLOW_RECORD && PINN_FLOW_STATE == FLOW_STATE, "flow record / state size mismatch");
  if (int rc = flow_grid("pinn_flow_stats", nx, ny, fields, npad)) return rc;
  if (capacity < 1 || capacity > (int64_t)1 << 30) return fail(-22, "pinn_flow_stats: capacity must be 1..2^30 (got %s%ld)", "", (long)capacity);
  if (every < 1) return fail(-22, "pinn_flow_stats: every must be >= 1 (got %s%ld)", "", (long)every);
  if (!(eps >= 0.0 && std::isfinite(eps))) return fail(-22, "pinn_flow_stats: eps must be finite and >= 0%s");
  if (!(t == -1.0 || (t >= 0.0 && std::isfinite(t)))) return fail(-22, "pinn_flow_stats: t must be -1 (the cadence) or finite and >= 0%s");
  if (!xs || !ys || !psi || !scratch || !state || !ring) return fail(-22, "pinn_flow_stats: null argument%s");
  if (misaligned(xs, 8) || misaligned(ys, 8) || misaligned(scratch, 8) || misaligned(state, 8) || misaligned(ring, 8))
    return fail(-22, "pinn_flow_stats: xs, ys, scratch, state and ring must be 8-byte aligned%s");
  if (misaligned(psi, 16)) return fail(-22, "pinn_flow_stats: psi must be 16-byte aligned%s");
  FlowStatsArgs a;
  a.nx = (long)nx; a.ny = (long)ny; a.npad = (long)npad; a.capacity = (long)capacity; a.fld = fields;
  a.xs = xs; a.ys = ys; a.psi = psi; a.eps = eps; a.t = t; a.every = (double)every;
  a.scratch = scratch; a.state = state; a.ring = ring;
  int rc = launch_flow_stats(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_flow_stats") : 0;
}

// ---- viscosity identification (visc.hip) ----
int64_t pinn_visc_scratch_bytes(int64_t n) {
  return n < 1 || n > (int64_t)1 << 30 ? -1 : (int64_t)visc_scratch_bytes((long)n);
}

int pinn_visc_grad(int64_t n, const float* fields, int64_t npad, const float* lap, const float* w, double w4,
                   float* sum_out, double* scratch, void* stream) {
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_visc_grad: n must be 1..2^30 (got %s%ld)", "", (long)n);
  if (!fields || !lap || !sum_out || !scratch) return fail(-22, "pinn_visc_grad: null argument%s");
  if (npad < n || npad % 4 != 0) return fail(-22, "pinn_visc_grad: npad must be >= n and a multiple of 4%s");
  if (!(w4 >= 0.0) || !std::isfinite(w4)) return fail(-22, "pinn_visc_grad: w4 must be finite and >= 0%s");
  if (misaligned(fields, 16) || misaligned(lap, 16) || misaligned(w, 16))
    return fail(-22, "pinn_visc_grad: fields, lap and w must be 16-byte aligned%s");
  if (misaligned(sum_out, 4) || misaligned(scratch, 8))
    return fail(-22, "pinn_visc_grad: sum_out must be 4-byte aligned, scratch 8-byte%s");
  ViscGradArgs a;
  a.n = (long)n; a.npad = (long)npad; a.fld = fields; a.lap = lap; a.w = w; a.w4 = w4; a.sum_out = sum_out; a.scratch = scratch;
  int rc = launch_visc_grad(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_visc_grad") : 0;
}

int pinn_visc_update(const float* sum, double coef, double lr, double beta1, double beta2, double eps, double theta_min,
                     double theta_max, double* state, float* nu_dev, void* stream) {
  static_assert(PINN_VISC_STATE == VISC_STATE, "viscosity state size mismatch");
  if (!sum || !state || !nu_dev) return fail(-22, "pinn_visc_update: null argument%s");
  if (misaligned(sum, 4) || misaligned(nu_dev, 4) || misaligned(state, 8))
    return fail(-22, "pinn_visc_update: sum and nu_dev must be 4-byte aligned, state 8-byte%s");
  if (!std::isfinite(coef) || !std::isfinite(lr) || lr < 0.0) return fail(-22, "pinn_visc_update: coef must be finite, lr finite and >= 0%s");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0) || !std::isfinite(eps))
    return fail(-22, "pinn_visc_update: betas must lie in [0, 1), eps must be finite and > 0%s");
  if (!std::isfinite(theta_min) || !std::isfinite(theta_max) || !(theta_min <= theta_max))
    return fail(-22, "pinn_visc_update: theta_min <= theta_max, both finite%s");
  ViscUpdateArgs a;
  a.sum = sum; a.coef = coef; a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
  a.theta_min = theta_min; a.theta_max = theta_max; a.state = state; a.nu_dev = nu_dev;
  int rc = launch_visc_update(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_visc_update") : 0;
}

// ---- Reynolds-number continuation (visc_sched.hip) ----
static int check_visc_schedule(const char* what, const pinn_visc_schedule_t* s) {
  if (!s) return fail(-22, "%s: null schedule", what);
  if (s->shape < PINN_RAMP_GEOMETRIC || s->shape > PINN_RAMP_LINEAR_NU) return fail(-22, "%s: unknown shape %ld", what, (long)s->shape);
  if (s->updates <= 0) return fail(-22, "%s: updates must be > 0 (got %ld)", what, (long)s->updates);
  if (s->hold < 0) return fail(-22, "%s: hold must be >= 0 (got %ld)", what, (long)s->hold);
  if (s->stairs < 0) return fail(-22, "%s: stairs must be >= 0 (got %ld)", what, (long)s->stairs);
  if (!std::isfinite(s->re_start) || !(s->re_start > 0.0)) return fail(-22, "%s: re_start must be finite and > 0", what);
  if (!std::isfinite(s->re_end) || !(s->re_end > 0.0)) return fail(-22, "%s: re_end must be finite and > 0", what);
  if (!std::isfinite(s->nu_start) || !(s->nu_start > 0.f) || !std::isfinite(s->nu_end) || !(s->nu_end > 0.f))
    return fail(-22, "%s: nu_start and nu_end must be finite and > 0", what);
  if (!std::isfinite(s->cap_factor) || s->cap_factor < 0.0) return fail(-22, "%s: cap_factor must be finite and >= 0", what);
  if (s->cap_factor > 0.0 && (!std::isfinite(s->cap_start) || !(s->cap_start > 0.f) || !std::isfinite(s->cap_end) || !(s->cap_end > 0.f)))
    return fail(-22, "%s: cap_start and cap_end must be finite and > 0 with a cap_factor", what);
  return 0;
}

double pinn_visc_schedule_value(const pinn_visc_schedule_t* schedule, int64_t t, double* record6) {
  static_assert(PINN_RAMP_RECORD == 6, "continuation record size mismatch");
  if (check_visc_schedule("pinn_visc_schedule_value", schedule)) return NAN;
  if (t < 0) { fail(-22, "pinn_visc_schedule_value: t must be >= 0%s"); return NAN; }
  const ViscRampValue r = visc_schedule_value(*schedule, (long long)t);
  if (record6) visc_schedule_record(r, (long long)t, record6);
  return (double)r.nu;
}

int pinn_visc_schedule_step(const pinn_visc_schedule_t* schedule, int64_t* pos, float* nu_dev, float* cap_dev,
                            double* record, void* stream) {
  if (int rc = check_visc_schedule("pinn_visc_schedule_step", schedule)) return rc;
  if (!pos || !nu_dev || !record) return fail(-22, "pinn_visc_schedule_step: null argument%s");
  if (misaligned(pos, 8) || misaligned(record, 8) || misaligned(nu_dev, 4) || misaligned(cap_dev, 4))
    return fail(-22, "pinn_visc_schedule_step: pos and record must be 8-byte aligned, nu_dev and cap_dev 4-byte%s");
  if (cap_dev && !(schedule->cap_factor > 0.0)) return fail(-22, "pinn_visc_schedule_step: cap_dev needs a cap_factor > 0%s");
  ViscSchedArgs a;
  a.sched = *schedule; a.pos = reinterpret_cast<long long*>(pos); a.nu_dev = nu_dev; a.cap_dev = cap_dev; a.record = record;
  int rc = launch_visc_sched(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_visc_schedule_step") : 0;
}

// ---- convergence monitor (monitor.hip) ----
int64_t pinn_monitor_scratch_bytes(void) { return (int64_t)monitor_scratch_bytes(); }

int pinn_monitor_vis_stats(int64_t n, const float* vis_t, float vis_t0, float* sum_out, double* info, double* scratch,
                           void* stream) {
  static_assert(PINN_MON_INFO == MON_INFO, "monitor info size mismatch");
  if (n < 1 || n > (int64_t)1 << 30) return fail(-22, "pinn_monitor_vis_stats: n must be 1..2^30 (got %s%ld)", "", (long)n);
  if (!vis_t || !sum_out || !info || !scratch) return fail(-22, "pinn_monitor_vis_stats: null argument%s");
  if (misaligned(vis_t, 16)) return fail(-22, "pinn_monitor_vis_stats: vis_t must be 16-byte aligned%s");
  if (misaligned(sum_out, 4) || misaligned(info, 8) || misaligned(scratch, 8))
    return fail(-22, "pinn_monitor_vis_stats: sum_out must be 4-byte aligned, info and scratch 8-byte%s");
  MonVisArgs a;
  a.n = (long)n; a.vis_t = vis_t; a.vis_t0 = vis_t0; a.sum_out = sum_out; a.info = info; a.scratch = scratch;
  int rc = launch_monitor_vis_stats(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_monitor_vis_stats") : 0;
}

int pinn_monitor_observe(const float* eq, const float* bc, const float* sup, const float* lam, double alpha_b,
                         double alpha_s, double alpha_e, double eq4_weight, double n_eq, double n_b, double n_s, double n_p,
                         double Re, const pinn_monitor_config_t* cfg, double* state, double* ring, void* stream) {
  static_assert(PINN_MON_RECORD == MON_RECORD && PINN_MON_STATE == MON_STATE, "monitor record / state size mismatch");
  static_assert((int)PINN_MON_STOP_PLATEAU == MON_STOP_PLATEAU && (int)PINN_MON_STOP_RE_EFF == MON_STOP_RE_EFF &&
                (int)PINN_MON_STOP_NONFINITE == MON_STOP_NONFINITE, "monitor stop bits mismatch");
  if (!cfg) return fail(-22, "pinn_monitor_observe: null configuration%s");
  // the configuration first: it needs no device
  if (cfg->every < 1) return fail(-22, "pinn_monitor_observe: every must be >= 1 (got %s%ld)", "", (long)cfg->every);
  if (cfg->window < 1) return fail(-22, "pinn_monitor_observe: window must be >= 1 (got %s%ld)", "", (long)cfg->window);
  if (cfg->patience < 1) return fail(-22, "pinn_monitor_observe: patience must be >= 1 (got %s%ld)", "", (long)cfg->patience);
  if (cfg->capacity < 1 || cfg->capacity > (int64_t)1 << 30)
    return fail(-22, "pinn_monitor_observe: capacity must be 1..2^30 (got %s%ld)", "", (long)cfg->capacity);
  if (cfg->min_updates < 0) return fail(-22, "pinn_monitor_observe: min_updates must be >= 0 (got %s%ld)", "", (long)cfg->min_updates);
  if (cfg->quantity < 0 || cfg->quantity > 2) return fail(-22, "pinn_monitor_observe: quantity must be 0..2 (got %s%ld)", "", (long)cfg->quantity);
  if (cfg->plateau_on && !(std::isfinite(cfg->min_rel_improvement) && cfg->min_rel_improvement >= 0.0))
    return fail(-22, "pinn_monitor_observe: min_rel_improvement must be finite and >= 0%s");
  if (cfg->re_eff_on && !(std::isfinite(cfg->re_eff_tol) && cfg->re_eff_tol >= 0.0))
    return fail(-22, "pinn_monitor_observe: re_eff_tol must be finite and >= 0%s");
  if (cfg->re_eff_on && !cfg->ev) return fail(-22, "pinn_monitor_observe: re_eff_on needs the ev flavour (there is no vis_t)%s");
  if (!(n_eq >= 1.0 && std::isfinite(n_eq)) || !(n_b >= 1.0 && std::isfinite(n_b)))
    return fail(-22, "pinn_monitor_observe: n_eq and n_b must be finite and >= 1%s");
  if (!(n_s >= 0.0 && std::isfinite(n_s)) || !(n_p >= 0.0 && std::isfinite(n_p)))
    return fail(-22, "pinn_monitor_observe: n_s and n_p must be finite and >= 0%s");
  if (!(Re > 0.0 && std::isfinite(Re))) return fail(-22, "pinn_monitor_observe: Re must be finite and > 0%s");
  if (!eq || !bc || !state || !ring) return fail(-22, "pinn_monitor_observe: null argument%s");
  if (misaligned(eq, 4) || misaligned(bc, 4) || misaligned(sup, 4) || misaligned(lam, 4) || misaligned(state, 8) ||
      misaligned(ring, 8))
    return fail(-22, "pinn_monitor_observe: the sums and lam must be 4-byte aligned, state and ring 8-byte%s");
  MonObserveArgs a;
  a.eq = eq; a.bc = bc; a.sup = sup; a.lam = lam;
  a.alpha_b = alpha_b; a.alpha_s = alpha_s; a.alpha_e = alpha_e; a.w4 = eq4_weight;
  a.n_eq = n_eq; a.n_b = n_b; a.n_s = n_s; a.n_p = n_p; a.Re = Re;
  a.every = (long)cfg->every; a.window = (long)cfg->window; a.patience = (long)cfg->patience;
  a.min_updates = (long)cfg->min_updates; a.capacity = (long)cfg->capacity;
  a.quantity = cfg->quantity; a.ev = cfg->ev != 0; a.plateau_on = cfg->plateau_on != 0; a.re_on = cfg->re_eff_on != 0;
  a.min_rel = cfg->min_rel_improvement; a.re_tol = cfg->re_eff_tol;
  a.state = state; a.ring = ring;
  int rc = launch_monitor_observe(a, (hipStream_t)stream);
  return rc ? hipfail(rc, "pinn_monitor_observe") : 0;
}


// ---- training-state snapshots (state.hip) ----
int64_t pinn_state_scratch_bytes(void) { return (int64_t)state_scratch_bytes(); }

int64_t pinn_state_layout(int nseg, const int64_t* bytes, int64_t* offsets_out) {
  if (nseg < 0 || (nseg > 0 && (!bytes || !offsets_out))) { fail(-22, "pinn_state_layout: bad argument%s"); return -1; }
  int64_t end = 0;
  for (int k = 0; k < nseg; ++k) {
    if (bytes[k] < 0 || bytes[k] % 4 != 0 || bytes[k] > (int64_t)1 << 46) {
      fail(-22, "pinn_state_layout: a segment size must be a multiple of 4 in 0..2^46 (got %s%ld)", "", (long)bytes[k]);
      return -1;
    }
    offsets_out[k] = end = (end + 255) / 256 * 256;
    end += bytes[k];
  }
  return end;
}

int pinn_state_digest_host(const void* ptr, int64_t bytes, uint64_t* out2) {
  if (bytes < 0 || bytes % 4 != 0) return fail(-22, "pinn_state_digest_host: the size must be a multiple of 4 and >= 0 (got %s%ld)", "", (long)bytes);
  if ((bytes > 0 && !ptr) || !out2) return fail(-22, "pinn_state_digest_host: null argument%s");
  unsigned long long d[2];
  state_digest_host(ptr, (unsigned long long)bytes, d);
  out2[0] = d[0]; out2[1] = d[1];
  return 0;
}

// pack (live != NULL table of sources) or unpack (table of destinations): checks, then one launch per STATE_MAX_SEG segments
static int state_copy(const char* what, bool pack, int nseg, void* const* live, const int64_t* bytes, const int64_t* offsets,
                      void* staging, int64_t staging_bytes, uint64_t* digests, void* scratch, void* stream) {
  if (nseg < 1 || nseg > 1 << 16) return fail(-22, "%s: nseg must be 1..65536 (got %ld)", what, (long)nseg);
  if (!live || !bytes || !offsets || !digests || !scratch) return fail(-22, "%s: null argument", what);
  if (misaligned(digests, 8) || misaligned(scratch, 8)) return fail(-22, "%s: digests_out and scratch must be 8-byte aligned", what);
  if (misaligned(staging, 16)) return fail(-22, "%s: the staging buffer must be 16-byte aligned", what);
  int64_t end = 0;
  for (int k = 0; k < nseg; ++k) {
    if (bytes[k] < 0 || bytes[k] % 4 != 0 || bytes[k] > (int64_t)1 << 46)
      return fail(-22, "%s: a segment size must be a multiple of 4 in 0..2^46 (got %ld)", what, (long)bytes[k]);
    if (bytes[k] > 0 && (!live[k] || misaligned(live[k], 4)))
      return fail(-22, "%s: segment %ld has bytes but no buffer, or one that is not 4-byte aligned", what, (long)k);
    if (offsets[k] == -1 || bytes[k] == 0) continue;            // digest only, or empty: nothing in the staging buffer
    if (offsets[k] < end || offsets[k] % 256 != 0 || !staging || offsets[k] + bytes[k] > staging_bytes)
      return fail(-22, "%s: the offset of segment %ld is not a multiple of 256, overlaps the segment before it or runs past the staging buffer",
                  what, (long)k);
    end = offsets[k] + bytes[k];
  }
  for (int k0 = 0; k0 < nseg; k0 += STATE_MAX_SEG) {
    StateArgs a;
    memset(&a, 0, sizeof(a));
    a.nseg = nseg - k0 < STATE_MAX_SEG ? nseg - k0 : STATE_MAX_SEG;
    a.digests = reinterpret_cast<unsigned long long*>(digests) + 2 * (size_t)k0;
    a.scratch = static_cast<double*>(scratch);
    for (int j = 0; j < a.nseg; ++j) {
      const int k = k0 + j;
      char* st = offsets[k] == -1 || bytes[k] == 0 ? nullptr : static_cast<char*>(staging) + offsets[k];
      StateSeg& s = a.seg[j];
      s.bytes = (unsigned long long)bytes[k];
      s.chunk0 = a.nchunks;
      a.nchunks += state_chunks(s.bytes);
      if (st) {                                                  // the padding stops at the buffer's end (the last segment)
        const int64_t e = offsets[k] + bytes[k], lim = (e + 255) / 256 * 256;
        s.pad = (unsigned long long)((lim < staging_bytes ? lim : staging_bytes) - e);
      }
      if (pack) { s.rd = live[k]; s.wr = st; }                   // st NULL: the source is digested, nothing is stored
      else if (st) { s.rd = st; s.wr = live[k]; }
      else { s.rd = live[k]; s.wr = nullptr; }                   // the live buffer is digested, nothing is written
    }
    int rc = launch_state_copy(a, pack, (hipStream_t)stream);
    if (rc) return hipfail(rc, what);
  }
  return 0;
}

int pinn_state_pack(int nseg, const void* const* src, const int64_t* bytes, const int64_t* offsets, void* dst, int64_t dst_bytes,
                    uint64_t* digests_out, void* scratch, void* stream) {
  return state_copy("pinn_state_pack", true, nseg, const_cast<void* const*>(src), bytes, offsets, dst, dst_bytes, digests_out,
                    scratch, stream);
}

int pinn_state_unpack(int nseg, const void* src, int64_t src_bytes, const int64_t* bytes, const int64_t* offsets, void* const* dst,
                      uint64_t* digests_out, void* scratch, void* stream) {
  return state_copy("pinn_state_unpack", false, nseg, dst, bytes, offsets, const_cast<void*>(src), src_bytes, digests_out, scratch,
                    stream);
}

}  // extern "C"
