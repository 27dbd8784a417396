// Host engine of libmmt_hip.so: parameter layout, workspace plan and the forward / backward
// launch sequence of the multimodal transformer training step, behind the C-ABI of include/mmt.h.
//
// Reference structure restated (model.py): per layer, per modality i
//   x1 = x0 + proj(MHA(LN1 x0))           MHA heads: q/k/v = Linear(C,hs/2)+tanh+Linear(hs/2,hs)
//   x2 = x1 + FFN(LN2 x1)                 FFN = Linear(C,4C)+ReLU+Linear(4C,C)
//   x3 = x2 + proj(CA(LNc x2, [x2_j]))    only for cross modalities; one softmax per KV stream, summed
// post: logits = Linear(V/2,V)(tanh(Linear(C,V/2)(LNf x))), loss = mean CE.
// All modalities' identical-shape ops run as ONE grouped launch (blockIdx.z = modality).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mmt.h"
#include "mmt_common.h"
#include "mmt_gemm_plan.h"
#include "mmt_attn_plan.h"
#include "mmt_kernels.h"

namespace {

constexpr int MAXM = MMT_MAX_MODALITIES;

inline int64_t rup(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline int r8(int x) { return (int)rup(x < 1 ? 1 : x, 8); }

struct Mat {
  int64_t off = -1;  // fp32 offset of the [rows, cols] weight in the flat param buffer
  int rows = 0, cols = 0;
  int64_t pk = 0;    // bf16 element offset in the packed-weight region
  int ld = 0;        // packed leading dimension (multiple of 8)
  // MX-fp8 copy (precision fp8): byte offsets of the e4m3fn rows and E8M0 exponents in the fp8
  // pack region, row strides in bytes; pk8 < 0: no fp8 copy
  int64_t pk8 = -1, ps8 = -1;
  int ld8 = 0, lds8 = 0;
};

struct TensorInfo {
  std::string name;
  int64_t off;
  int nd;
  int64_t shape[2];
  int kind;
};

struct LM {  // parameters of one (layer, modality)
  int64_t ln1w, ln1b, ln2w, ln2b;
  Mat W1; int64_t b1; int64_t w2;
  Mat P0; int64_t bp0; Mat P2; int64_t bp2;
  Mat F0; int64_t bf0; Mat F2; int64_t bf2;
  bool cross = false;  // cross-attention active (cross flag and M > 1)
  int64_t lncw = -1, lncb = -1;
  Mat Wq; Mat Wkv[MAXM]; Mat C0; int64_t bc0 = -1; Mat C2; int64_t bc2 = -1;
};

struct PostM {
  int64_t lnw, lnb;
  Mat H0; int64_t b0; Mat H2; int64_t b2;
  int64_t tok;
};

struct ActLM {  // byte offsets of one (layer, modality)'s saved activations in the workspace
  size_t a, mean1, rstd1, h1, qkv, o, lse, p1, x1, c, mean2, rstd2, f, x2, x2h;
  size_t d, meanc, rstdc, qc, kv[MAXM], oc, ocj[MAXM], lsej[MAXM], pc, x3;
  size_t dm, dmj[MAXM];  // attention dropout keep bits (SA; CA per KV stream), dropout > 0 only
  // MX-fp8 copies of the fp8 GEMMs' A operands (precision fp8): LN1 / LN2 / LNc outputs and the
  // FFN hidden, e4m3fn bytes + E8M0 exponents
  size_t a8 = 0, as8 = 0, c8 = 0, cs8 = 0, f8 = 0, fs8 = 0, d8 = 0, ds8 = 0;
  size_t fm = 0;  // ReLU bits of the FFN hidden [R][4C / 8] (the ffn2 data gradient's ReLU')
};

struct Plan {
  int B = -1;
  size_t total = 0;
  size_t pack = 0;
  size_t slab = 0, slab_bytes = 0;  // split-K slabs of the weight-gradient GEMMs
  size_t flag = 0;                  // int32 non-finite-loss bitmask (bit i: modality i)
  size_t pack8 = 0;                 // MX-fp8 weight copies (precision fp8)
  std::vector<ActLM> act;  // [L*M]
  size_t xemb[MAXM];
  size_t lnf16[MAXM], meanf[MAXM], rstdf[MAXM], hh[MAXM], dlog[MAXM];
  // backward scratch, per modality. The data gradients a side-stream weight-gradient GEMM reads
  // (gbig, gq, gh1, gp, gpc, dkv) have two copies, one per backward-stage parity, so the main
  // stream may run a whole stage ahead of the side stream (mmt_backward joins once, at its end)
  size_t dres[MAXM], dln[MAXM], gdo[MAXM], gqkv[MAXM];
  size_t gbig[2][MAXM], gq[2][MAXM], gh1[2][MAXM], gp[2][MAXM], gpc[2][MAXM];
  // bf16 residual-gradient copies, rotated over 8 buffers (one per LayerNorm-backward / copy launch,
  // three per layer stage): a side-stream weight-gradient GEMM up to one stage behind still reads
  // its copy when the main stream writes the next ones
  size_t dres16[8][MAXM];
  size_t dvec[MAXM][MAXM];
  size_t dkv[2][MAXM][MAXM];
  size_t celoss[MAXM];  // float [512]: the cross-entropy blocks' loss shares (summed in block order)
  const void* gh1_pad_ws = nullptr;  // the workspace whose gh1 pad columns (written by no kernel) are zeroed
  size_t eperm[MAXM];  // int [R]: the rows in token order for the token-table gradient (mmt_launch_emb_sort)
  // deterministic mode: partial-sum scratch of ONE producer launch (every producer runs on the main stream, in
  // stream order with its ordered sum, so one region serves them all); planned whatever the switch says
  size_t det = 0;
  int64_t det_floats = 0;
  // KV-cache decode (generate): compact [B, *] rows of ONE new position per sequence
  struct Dec {
    size_t x0, a16, mean, rstd, h1, qkv, o16, p1, f, x2h, d16, qc, oc, pc, lnf16, hh;
    size_t kv[MAXM];
  } dec[MAXM];
  std::vector<size_t> dec_x;  // [L*M][3]: fp32 residual stream x1, x2, x3 of the new rows
};

// Sample fan-out (mmt_decode_fanout_step): byte offsets in the caller's fan buffer. The compact scratch of
// B*S rows (what Plan::dec / dec_x are for B rows) and the tail caches: per (layer, modality) the self-attention
// tail [B*S, max_new, 3C], per (layer, cross modality, KV stream) the cross tail [B*S, max_new, 2C], bf16, row
// r*max_new + (pos - n0), columns as the forward's rows
struct FanPlan {
  int B = -1, S = -1, max_new = -1;
  size_t total = 0;
  Plan::Dec dec[MAXM];
  std::vector<size_t> dec_x;
  std::vector<size_t> sa_tail;  // [L*M]
  std::vector<size_t> ca_tail;  // [L*M][MAXM]
};

// Rolling-window step (mmt_rolling_step): the compact scratch of B*S*m rows in the caller's roll buffer, residual
// rows in two layer slots (dec_x [2*M][3]), and per modality the fp32 [B*S, C] rows the post block reads (the last
// tail row of every path)
struct RollPlan {
  size_t total = 0;
  Plan::Dec dec[MAXM];
  std::vector<size_t> dec_x;
  size_t last[MAXM];
};

}  // namespace

// Every MMT_* environment variable the engine reads, with its default and its meaning (DESIGN.md §3 has the same
// table). Read once, when the process first calls into the engine or a setter: nothing changes them after the
// library is loaded. The five knobs with a setter (include/mmt.h) only start from their variable.
namespace {
struct Knobs {
  // MMT_RELU_BITS / mmt_set_relu_bits: the FFN's ReLU' as bits written by ffn0 (16x fewer bytes than the bf16 hidden
  // the ffn2 data gradient reads back). Latched per context by mmt_create (the bit rows are allocated only then);
  // off by default: on the final round-5 build the bf16 aux measured faster (same box,
  // profiles/r5am_relu_bits_final_ab.txt: C1 8.502 -> 8.477 ms, target 19.770 -> 19.505 ms), where the first
  // version had been 0.1-0.7 % faster than the aux
  int relu_bits = mmt_env_int("MMT_RELU_BITS", 0);
  // MMT_DROP_COPY_FUSE / mmt_set_drop_copy_fuse: the FFN backward's dropout-masked bf16 residual-gradient copy (+ FFN
  // output-bias gradient) in the epilogue of the last cross-attention K/V dX launch into that gradient (1), or a
  // separate drop_copy pass for every modality (0)
  int drop_copy_fuse = mmt_env_int("MMT_DROP_COPY_FUSE", 1);
  // MMT_ATTN_QKV2 / mmt_set_attn_qkv2: hs 32, the Q/K/V stage-2 backward in the one-pass attention backward's
  // epilogue (1) or the separate qkv2 backward over the bf16 dQ / dK / dV (0); read at every step
  int attn_qkv2 = mmt_env_int("MMT_ATTN_QKV2", 1);
  // MMT_FFN_FUSED / mmt_set_ffn_fused: the FFN forward as one launch at C = 256 (include/mmt.h); read at every forward
  int ffn_fused = mmt_env_int("MMT_FFN_FUSED", 1);
  // MMT_ATTN_QKV_ONCHIP / mmt_set_attn_qkv_onchip: hs 32 self-attention at T <= 256 in training forwards: Q / K / V
  // made on chip from h1 and W2 (AttnProblem::oc_*) by the forward (bit 0) and by the one-pass backward (bit 1);
  // with both bits the stage-1 GEMM drops its stage-2 epilogue and the Q/K/V rows are never written. Latched by
  // mmt_forward
  int attn_qkv_onchip = mmt_env_int("MMT_ATTN_QKV_ONCHIP", 3) & 3;

  // MMT_LN_FUSE: 0 = no LayerNorm in a GEMM epilogue, backward (gemm_ln_bwd) or forward (MMT_LN_FUSE_FWD)
  int ln_fuse = mmt_env_int("MMT_LN_FUSE", 1);
  // MMT_LN_FUSE_FWD: the next LayerNorm's forward in the ffn2 residual GEMM's epilogue; bf16 at C == 256 (whole rows
  // per 256x256 tile). 2: also C = 512 (128 x 512 tile), measured slower on the 2-stage ring (target 20.09 ->
  // 20.43 ms, profiles/r3u_ab.txt)
  int ln_fuse_fwd = mmt_env_int("MMT_LN_FUSE_FWD", 1);
  // MMT_LN2_FUSE: ln2 in the fused out-projection's epilogue (0: the separate ln_fwd pass; fp8 keeps the pass, which
  // also writes the MX-fp8 copy)
  int ln2_fuse = mmt_env_int("MMT_LN2_FUSE", 1);
  // MMT_MLP2: the out-projection pair as one launch (Runner::mlp2). Forward fused by default: C1 8.80 -> 8.70 ms/step
  // (standalone 45.9 -> 43.0 us at C1, 119.6 -> 112.8 us at the target)
  int mlp2 = mmt_env_int("MMT_MLP2", 1);
  // MMT_MLP2_BWD: its backward pair: 2 = fused at C = 256 only, 1 = every width, 0 = never. Standalone the fused
  // backward measured 33.5 / 80.6 us against 29.3 / 61.6 us for the pair (C1 / target, tools/mlp2_bench.py; one
  // block per CU at 136 KiB of LDS with both B operands read transposed cannot hide what the two 2-3 blocks-per-CU
  // GEMMs overlap, profiles/r5h_*), but in the C1 step beside the side stream it wins: 7.975 / 7.982 -> 7.949 /
  // 7.960 ms (round 6, profiles/r6x_c1_env_ab.txt); at C = 512 it stays two GEMMs
  int mlp2_bwd = mmt_env_int("MMT_MLP2_BWD", 2);
  // MMT_QKV2_FUSE: the per-head Q/K/V stage 2 (model.py:39, 44, 49) in the stage-1 GEMM's epilogue at hs 32 / 64
  // (SURVEY.md K4); 0 keeps the separate kernel
  int qkv2_fuse = mmt_env_int("MMT_QKV2_FUSE", 1);
  // MMT_MASK_AHEAD: when the attention dropout keep bits are made. 0: all later layers' while layer 0 computes;
  // 1: layer l + 1's while layer l computes (one fork and one join per layer), so the masks overlap each layer's
  // attention forward instead of layer 0's GEMMs (C3 attention forward 394 -> 955 us live); 2: layer l + 1's bits
  // forked after layer l's self-attention forward, so they overlap that layer's GEMMs, which take the tile hint
  // until the next join, rather than its attention. Unset (-1): 1 from 12 layers on, where the later layers' pile
  // beside layer 0 grows past what one layer's GEMMs hide: C4 (24 layers) 312.4 -> 308.6 ms, C3 (12) 141.1 ->
  // 140.5-140.9, target (6) 19.07 -> 19.04, C1 (6) 7.87 -> 7.90 (profiles/r6ab_mask_ab.txt, r6ae_c4_mask_ab.txt)
  int mask_ahead = mmt_env_int("MMT_MASK_AHEAD", -1);
  // MMT_MASK_T2: main-stream GEMMs beside the keep-bit launches take the 128 x 256 tile (0: the ping-pong kernel
  // throughout)
  int mask_t2 = mmt_env_int("MMT_MASK_T2", 1);
  // MMT_DW_ATTN_SMALL=1: the FFN weight gradients (the side-stream launches still running when the self-attention
  // backward starts) on the 128 x 128 tile, whose 64 KiB of LDS leave room on their CUs for one of the attention
  // backward's 80 KiB workgroups
  int dw_attn_small = mmt_env_int("MMT_DW_ATTN_SMALL", 0);
  // MMT_FLUSH_HOLD=1: one side-stream fork per backward stage (every stage but the last layer's, whose weight
  // gradients would otherwise only start after its data-gradient chain, at the end of the step)
  int flush_hold = mmt_env_int("MMT_FLUSH_HOLD", 0);
  // MMT_SIDE_STREAM=0: everything on the caller's stream, no side stream is made
  int side_stream = mmt_env_int("MMT_SIDE_STREAM", 1);
  // MMT_SIDE_PRIORITY (optional): HIP stream priority of the side stream (lower = higher priority, clamped to the
  // device's range); unset = default priority
  const char* side_priority = getenv("MMT_SIDE_PRIORITY");
  // MMT_PROBE_EVENTS: event pairs mmt_probe_set makes for the recorded launches (recording stops when they run out)
  int probe_events = mmt_env_int("MMT_PROBE_EVENTS", 4096);
};
Knobs& knobs() {
  static Knobs k;
  return k;
}
int swap_knob(int& k, int v) {
  const int old = k;
  k = v;
  return old;
}
}  // namespace

extern "C" int mmt_set_relu_bits(int on) { return swap_knob(knobs().relu_bits, on); }
extern "C" int mmt_set_drop_copy_fuse(int on) { return swap_knob(knobs().drop_copy_fuse, on); }
extern "C" int mmt_set_attn_qkv2(int on) { return swap_knob(knobs().attn_qkv2, on); }
extern "C" int mmt_set_ffn_fused(int on) { return swap_knob(knobs().ffn_fused, on); }
extern "C" int mmt_set_attn_qkv_onchip(int bits) { return swap_knob(knobs().attn_qkv_onchip, bits & 3); }

struct mmt_ctx {
  mmt_config cfg;
  int M, C, H, L, T, hs, hh;
  int V[MAXM];
  bool any_cross = false;
  int ncross = 0;
  std::vector<TensorInfo> tensors;
  std::vector<LM> lm;  // [L*M]
  PostM post[MAXM];
  int64_t pos_off = 0;
  int64_t nparams = 0, nactive = 0;
  int64_t emb_begin = 0, emb_end = 0, post_begin = 0, post_end = 0;
  std::vector<int64_t> layer_begin, layer_end;
  // weight packing
  std::vector<PackSeg> segs;
  std::vector<int> tasks;
  // MX-fp8 weight copies (precision fp8): quantisation segments and the fp8 pack region size
  std::vector<MxSeg> mxsegs;
  int64_t pack8_bytes = 0;
  int mx_units = 0;
  MxSeg* d_mxsegs = nullptr;
  int tables_device = -1;
  bool fp8 = false;
  bool relu_bits = false;  // g_relu_bits at mmt_create
  // token-table gradient: the rows' sort runs at backward stage 0 on the side stream (it reads only the
  // forward's token ids); emb_ev marks its end for the embedding stage
  hipEvent_t emb_ev = nullptr;
  bool emb_sorted = false;
  int64_t pack_elems = 0;
  PackSeg* d_segs = nullptr;
  int* d_tasks = nullptr;
  // state
  Plan plan;
  int last_B = -1;
  bool fwd_ready = false;
  bool cache_ready = false;  // a forward filled the workspace's Q/K/V (decode may follow)
  // sample fan-out: the buffer plan and the run in progress (n0, samples, next position; fan_next < 0: none)
  FanPlan fan;
  int fan_n0 = -1, fan_S = -1, fan_next = -1;
  bool last_training = false;
  uint64_t step_counter = 0;
  // dropout: seed of the next training forward (mmt_set_dropout_seed) and of the last one
  uint64_t next_seed = 0;
  bool next_seed_set = false;
  uint64_t fwd_seed = 0;
  bool fwd_drop = false;
  const int64_t* last_idx[MAXM] = {};  // forward token ids, read by the embedding backward stage
  std::string err;
  // live kernel timing (mmt_probe_set): launch-label patterns and the HIP event pairs recorded
  // around every matching launch, with that launch's algorithmic flops / HBM bytes
  struct ProbeEv {
    hipEvent_t a, b;
    int pat;
    double flops, bytes;
  };
  std::vector<std::string> probe_pats;
  bool probe_on = true;
  std::vector<ProbeEv> probe_events;  // recorded launches (events taken from probe_pool in order)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> probe_pool;  // created by mmt_probe_set, not in the timed loop
  int ldv[MAXM], ldvh[MAXM];
  // backward side stream: the weight-gradient GEMMs (nothing in the data-gradient chain reads
  // them) run there, overlapping the latency-bound data-gradient kernels; joined at stage ends
  hipStream_t side = nullptr;
  int side_device = -1;
  bool side_off = false;  // mmt_set_side_stream(ctx, 0): this context runs everything on the caller's stream
  bool side_off_req = false;  // the requested setting, latched into side_off by the next mmt_forward (a
                              // forward and its backward always see one setting: work forked to the side
                              // stream is always joined)
  // mmt_backward (all stages in one call): no join per stage; the side stream's work of stage t is
  // recorded in stage_ev[t & 1] and the main stream waits for it only at the start of stage t + 2,
  // the first stage that rewrites that parity's scratch (Plan). mmt_backward_stage called alone (the
  // data-parallel path: each stage's gradient range must be final for its all-reduce) joins per stage.
  bool defer_join = false;
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  std::vector<hipEvent_t> evpool;
  size_t evnext = 0;
  int d16 = 0;  // rotation index of the current dres16 copy (reset at backward stage 0)
  // deterministic mode (mmt_set_deterministic; mmt_det.h): every arrival-order float sum of the backward leaves
  // its kernel as per-block partials (Plan::det) that one ordered sum adds. det_req is the requested setting,
  // latched into det by the next mmt_forward (a forward and its backward always run under one setting)
  bool det = false;
  bool det_req = false;
  // mmt_set_grad_accumulate: stage 0 of the backward leaves `grads` as it is (every writer adds)
  bool grad_accum = false;
  // on-chip self-attention Q/K/V (mmt_set_attn_qkv_onchip): onchip_req is the knob as mmt_forward found it (0
  // for a training == 0 forward, whose saved Q/K/V are the decode cache); onchip is what the forward's layers
  // then ran with (0 where the path does not apply), and its backward follows it. 3: Q/K/V were not written
  int onchip_req = 0, onchip = 0;
  // the training objective (mmt_set_loss), read by every forward with targets; loss_on: some entry is not the
  // plain mean CE (off: run_forward launches exactly what it launched before the spec existed)
  mmt_loss_spec loss[MAXM] = {};
  bool loss_on = false;
};

namespace {

thread_local std::string g_create_err;

int fail(mmt_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                                             \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return fail(ctx, MMT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

// -------------------------------------------------------------------------------------------
// parameter layout
// -------------------------------------------------------------------------------------------
struct Builder {
  mmt_ctx* c;
  int64_t cur = 0;
  int64_t alloc(int64_t n) {
    const int64_t o = cur;
    cur += rup(n > 0 ? n : 0, 16);
    return o;
  }
  void tensor(const std::string& name, int64_t off, int nd, int64_t s0, int64_t s1, int kind) {
    TensorInfo t;
    t.name = name; t.off = off; t.nd = nd; t.shape[0] = s0; t.shape[1] = s1; t.kind = kind;
    c->tensors.push_back(t);
  }
  Mat mat(const std::string& name, int rows, int cols, bool emit = true) {
    Mat m;
    m.rows = rows; m.cols = cols;
    m.off = alloc((int64_t)rows * cols);
    m.ld = r8(cols);
    if (emit) tensor(name, m.off, 2, rows, cols, 0);
    return m;
  }
  int64_t vec(const std::string& name, int n, int kind) {
    const int64_t o = alloc(n);
    tensor(name, o, 1, n, 0, kind);
    return o;
  }
};

void build_cross_params(Builder& b, LM& x, const std::string& p, int C, int H, int hs, int nkv) {
  x.lncw = -1;
  x.Wq = b.mat("", H * hs, C, false);
  for (int h = 0; h < H; ++h)
    b.tensor(p + "heads." + std::to_string(h) + ".query.weight", x.Wq.off + (int64_t)h * hs * C, 2, hs, C, 0);
  for (int j = 0; j < nkv; ++j) {
    x.Wkv[j] = b.mat("", H * 2 * hs, C, false);
    for (int h = 0; h < H; ++h)
      b.tensor(p + "heads." + std::to_string(h) + ".kv_projections." + std::to_string(j) + ".weight",
               x.Wkv[j].off + (int64_t)h * 2 * hs * C, 2, 2 * hs, C, 0);
  }
  x.C0 = b.mat(p + "proj.0.weight", C / 2, hs * H);
  x.bc0 = b.vec(p + "proj.0.bias", C / 2, 1);
  x.C2 = b.mat(p + "proj.2.weight", C, C / 2);
  x.bc2 = b.vec(p + "proj.2.bias", C, 1);
}

void build_layout(mmt_ctx* c) {
  Builder b{c};
  const int C = c->C, H = c->H, hs = c->hs, hh = c->hh, M = c->M, L = c->L;
  c->emb_begin = b.cur;
  for (int i = 0; i < M; ++i) {
    c->post[i].tok = b.alloc((int64_t)c->V[i] * C);
    b.tensor("pre_block.token_embedding_tables." + std::to_string(i) + ".weight", c->post[i].tok, 2, c->V[i], C, 0);
  }
  c->pos_off = b.alloc((int64_t)c->T * C);
  b.tensor("pre_block.position_embedding_table.weight", c->pos_off, 2, c->T, C, 0);
  c->emb_end = b.cur;
  c->lm.resize((size_t)L * M);
  const char* kinds[3] = {"key", "query", "value"};
  for (int l = 0; l < L; ++l) {
    c->layer_begin.push_back(b.cur);
    const std::string bl = "blocks." + std::to_string(l) + ".";
    for (int i = 0; i < M; ++i) {
      LM& x = c->lm[(size_t)l * M + i];
      const std::string p = bl + "sa_layers." + std::to_string(i) + ".";
      x.W1 = b.mat("", 3 * H * hh, C, false);
      x.b1 = b.alloc(3 * H * hh);
      x.w2 = b.alloc((int64_t)3 * H * hs * hh);
      for (int k = 0; k < 3; ++k)
        for (int h = 0; h < H; ++h) {
          const std::string hp = p + "heads." + std::to_string(h) + "." + kinds[k] + ".";
          const int blk = k * H + h;
          b.tensor(hp + "0.weight", x.W1.off + (int64_t)blk * hh * C, 2, hh, C, 0);
          b.tensor(hp + "0.bias", x.b1 + (int64_t)blk * hh, 1, hh, 0, 1);
          b.tensor(hp + "2.weight", x.w2 + (int64_t)blk * hs * hh, 2, hs, hh, 0);
        }
      x.P0 = b.mat(p + "proj.0.weight", C / 2, hs * H);
      x.bp0 = b.vec(p + "proj.0.bias", C / 2, 1);
      x.P2 = b.mat(p + "proj.2.weight", C, C / 2);
      x.bp2 = b.vec(p + "proj.2.bias", C, 1);
    }
    for (int i = 0; i < M; ++i) {
      LM& x = c->lm[(size_t)l * M + i];
      const std::string p = bl + "ffwd_layers." + std::to_string(i) + ".net.";
      x.F0 = b.mat(p + "0.weight", 4 * C, C);
      x.bf0 = b.vec(p + "0.bias", 4 * C, 1);
      x.F2 = b.mat(p + "2.weight", C, 4 * C);
      x.bf2 = b.vec(p + "2.bias", C, 1);
    }
    for (int i = 0; i < M; ++i) {
      LM& x = c->lm[(size_t)l * M + i];
      x.ln1w = b.vec(bl + "ln1_layers." + std::to_string(i) + ".weight", C, 2);
      x.ln1b = b.vec(bl + "ln1_layers." + std::to_string(i) + ".bias", C, 3);
      x.ln2w = b.vec(bl + "ln2_layers." + std::to_string(i) + ".weight", C, 2);
      x.ln2b = b.vec(bl + "ln2_layers." + std::to_string(i) + ".bias", C, 3);
    }
    for (int i = 0; i < M; ++i) {
      LM& x = c->lm[(size_t)l * M + i];
      if (!(c->cfg.cross_attention[i] && M > 1)) continue;
      x.cross = true;
      const std::string p = bl + "cross_attention_layers." + std::to_string(i) + ".";
      build_cross_params(b, x, p, C, H, hs, M - 1);
      x.lncw = b.vec(bl + "ln_cross_layers." + std::to_string(i) + ".weight", C, 2);
      x.lncb = b.vec(bl + "ln_cross_layers." + std::to_string(i) + ".bias", C, 3);
    }
    c->layer_end.push_back(b.cur);
  }
  c->post_begin = b.cur;
  for (int i = 0; i < M; ++i) {
    c->post[i].lnw = b.vec("post_block.fin_norm_layers." + std::to_string(i) + ".weight", C, 2);
    c->post[i].lnb = b.vec("post_block.fin_norm_layers." + std::to_string(i) + ".bias", C, 3);
  }
  for (int i = 0; i < M; ++i) {
    const std::string p = "post_block.soft_score_layers." + std::to_string(i) + ".";
    const int V = c->V[i], V2 = V / 2;
    c->post[i].H0 = b.mat(p + "0.weight", V2, C);
    c->post[i].b0 = b.vec(p + "0.bias", V2, 1);
    c->post[i].H2 = b.mat(p + "2.weight", V, V2);
    c->post[i].b2 = b.vec(p + "2.bias", V, 1);
  }
  c->post_end = b.cur;
  c->nactive = b.cur;
  // parameters that never receive a gradient: a CrossAttention built with zero KV modalities (M == 1,
  // model.py:198-200, 238). torch's AdamW skips them (no decay): they live past the active prefix.
  for (int l = 0; l < L; ++l)
    for (int i = 0; i < M; ++i) {
      if (!(c->cfg.cross_attention[i] && M == 1)) continue;
      LM dummy;
      const std::string bl = "blocks." + std::to_string(l) + ".";
      build_cross_params(b, dummy, bl + "cross_attention_layers." + std::to_string(i) + ".", C, H, hs, 0);
      b.vec(bl + "ln_cross_layers." + std::to_string(i) + ".weight", C, 2);
      b.vec(bl + "ln_cross_layers." + std::to_string(i) + ".bias", C, 3);
    }
  c->nparams = b.cur;

  // packed bf16 weights: every GEMM weight matrix with a padded leading dimension
  int64_t pk = 0;
  auto add = [&](Mat& m) {
    if (m.off < 0 || m.rows == 0) return;
    m.pk = pk;
    pk += rup((int64_t)m.rows * m.ld, 64);
    PackSeg s;
    s.src_off = m.off; s.dst_off = m.pk; s.rows = m.rows; s.cols = m.cols; s.dld = m.ld; s.pad_ = 0;
    const int si = (int)c->segs.size();
    c->segs.push_back(s);
    for (int r0 = 0; r0 < m.rows; r0 += 32) { c->tasks.push_back(si); c->tasks.push_back(r0); }
  };
  for (auto& x : c->lm) {
    add(x.W1); add(x.P0); add(x.P2); add(x.F0); add(x.F2);
    if (x.cross) {
      add(x.Wq);
      for (int j = 0; j < M - 1; ++j) add(x.Wkv[j]);
      add(x.C0); add(x.C2);
    }
  }
  for (int i = 0; i < M; ++i) { add(c->post[i].H0); add(c->post[i].H2); }
  c->pack_elems = pk;
  if (c->fp8) {
    // MX-fp8 copies of the weights of the fp8 forward GEMMs (Q/K/V stage 1, FFN, cross query)
    int64_t b8 = 0;
    auto add8 = [&](Mat& m) {
      if (m.off < 0 || m.rows == 0) return;
      m.ld8 = (int)rup(m.cols, 16);
      m.lds8 = (int)rup((m.cols + 31) / 32, 4);
      m.pk8 = b8;
      b8 += rup((int64_t)m.rows * m.ld8, 256);
      m.ps8 = b8;
      b8 += rup((int64_t)m.rows * m.lds8, 256);
      MxSeg sg{};
      sg.src = m.off; sg.dst = m.pk8; sg.sdst = m.ps8; sg.rows = m.rows; sg.cols = m.cols; sg.ld_src = m.cols;
      sg.ld8 = m.ld8; sg.lds8 = m.lds8;
      c->mxsegs.push_back(sg);
      c->mx_units = std::max(c->mx_units, m.rows * m.lds8);
    };
    for (auto& x : c->lm) {
      add8(x.W1); add8(x.F0); add8(x.F2);
      if (x.cross) add8(x.Wq);
    }
    c->pack8_bytes = b8;
  }
  for (int i = 0; i < M; ++i) {
    c->ldv[i] = r8(c->V[i]);
    c->ldvh[i] = r8(c->V[i] / 2);
  }
}

// -------------------------------------------------------------------------------------------
// workspace plan for batch B
// -------------------------------------------------------------------------------------------
// the non-finite-loss flag words sit right after the packed weights, at the same offset for every
// batch size, so querying them never replaces the plan of a pending backward / decode
size_t flag_offset(const mmt_ctx* c) { return (size_t)rup(c->pack_elems * 2, 256); }
// ... and in the same 256-byte block, behind the two words: one double per modality, the loss denominators D of
// mmt_set_loss (written by ce_denom, read by the loss kernel of the same forward)
constexpr size_t LOSS_DENOM_OFF = 64;
static_assert(LOSS_DENOM_OFF + sizeof(double) * MAXM <= 256, "the loss denominators fit the flag block");

// -------------------------------------------------------------------------------------------
// workspace plan for batch B (continued)
// -------------------------------------------------------------------------------------------
// the compact [rows, *] scratch of one decode step, every modality (rows = B, or B*S in a fan buffer)
// xlayers: the layers whose residual rows are kept apart (every layer; the rolling step rotates over two)
template <class Alloc>
void plan_dec_rows(mmt_ctx* c, Alloc& A, size_t B, Plan::Dec* dec, std::vector<size_t>& dec_x, int xlayers) {
  const int C = c->C, M = c->M, H = c->H;
  const size_t f4 = 4, b2 = 2;
  const int ldh1 = r8(3 * H * c->hh), ldp = r8(C / 2);
  dec_x.resize((size_t)xlayers * M * 3);
  for (int i = 0; i < M; ++i) {
    Plan::Dec& d = dec[i];
    d.x0 = A(B * C * f4); d.a16 = A(B * C * b2); d.mean = A(B * f4); d.rstd = A(B * f4);
    d.h1 = A(B * ldh1 * b2); d.qkv = A(B * 3 * C * b2); d.o16 = A(B * C * b2); d.p1 = A(B * ldp * b2);
    d.f = A(B * 4 * C * b2); d.x2h = A(B * C * b2); d.d16 = A(B * C * b2); d.qc = A(B * C * b2);
    d.oc = A(B * C * b2); d.pc = A(B * ldp * b2); d.lnf16 = A(B * C * b2); d.hh = A(B * c->ldvh[i] * b2);
    for (int j = 0; j < M - 1; ++j) d.kv[j] = A(B * 2 * C * b2);
  }
  for (auto& o : dec_x) o = A(B * C * f4);
}

// the fan buffer of mmt_decode_fanout_step (include/mmt.h); false when the sizes leave the launchers' int range
bool make_fan_plan(mmt_ctx* c, FanPlan& f, int B, int S, int max_new) {
  f = FanPlan();
  if (B < 1 || S < 1 || max_new < 1 || max_new >= c->T) return false;
  const int64_t rows = (int64_t)B * S;
  int64_t wide = 4 * (int64_t)c->C;
  for (int i = 0; i < c->M; ++i) wide = std::max<int64_t>(wide, c->ldv[i]);
  if (rows * wide >= ((int64_t)1 << 31)) return false;  // the GEMM and element kernels index rows * ld in int
  f.B = B; f.S = S; f.max_new = max_new;
  size_t cur = 0;
  auto A = [&](size_t bytes) { const size_t o = cur; cur += (size_t)rup((int64_t)bytes, 256); return o; };
  plan_dec_rows(c, A, (size_t)rows, f.dec, f.dec_x, c->L);
  const int M = c->M;
  f.sa_tail.assign((size_t)c->L * M, 0);
  f.ca_tail.assign((size_t)c->L * M * MAXM, 0);
  for (int l = 0; l < c->L; ++l)
    for (int i = 0; i < M; ++i) {
      f.sa_tail[(size_t)l * M + i] = A((size_t)rows * max_new * 3 * c->C * 2);
      if (c->lm[(size_t)l * M + i].cross)
        for (int j = 0; j < M - 1; ++j) f.ca_tail[((size_t)l * M + i) * MAXM + j] = A((size_t)rows * max_new * 2 * c->C * 2);
    }
  f.total = cur;
  return true;
}

// the buffer of mmt_rolling_step (include/mmt.h) for tails of m rows: the compact scratch of B*S*m rows and nothing
// else. The rows' own keys / values are that scratch's K|Q|V and cross-K/V rows of the layer in flight, and the
// residual rows of layer l live in slot l & 1, so the size does not depend on the number of layers
bool make_roll_plan(mmt_ctx* c, RollPlan& f, int B, int S, int m) {
  f = RollPlan();
  if (B < 1 || S < 1 || m < 1 || m >= c->T) return false;
  const int64_t rows = (int64_t)B * S * m;
  int64_t wide = 4 * (int64_t)c->C;
  for (int i = 0; i < c->M; ++i) wide = std::max<int64_t>(wide, c->ldv[i]);
  if ((int64_t)B * S >= ((int64_t)1 << 31) || rows * wide >= ((int64_t)1 << 31)) return false;  // as make_fan_plan
  size_t cur = 0;
  auto A = [&](size_t bytes) { const size_t o = cur; cur += (size_t)rup((int64_t)bytes, 256); return o; };
  plan_dec_rows(c, A, (size_t)rows, f.dec, f.dec_x, 2);
  for (int i = 0; i < c->M; ++i) f.last[i] = A((size_t)B * S * c->C * 4);
  f.total = cur;
  return true;
}

void make_plan(mmt_ctx* c, int B) {
  Plan& p = c->plan;
  p = Plan();
  p.B = B;
  size_t cur = 0;
  auto A = [&](size_t bytes) { const size_t o = cur; cur += (size_t)rup((int64_t)bytes, 256); return o; };
  const int64_t R = (int64_t)B * c->T;
  const int C = c->C, M = c->M, H = c->H;
  const size_t f4 = 4, b2 = 2;
  const int ldh1 = r8(3 * H * c->hh), ldp = r8(C / 2);
  const size_t bhT = (size_t)B * H * c->T;
  const size_t mbytes = c->cfg.dropout > 0.f ? (size_t)mmt_attn_mask_dwords(B, H, c->T) * 4 : 0;
  p.pack = A((size_t)c->pack_elems * b2);
  p.flag = A(256);  // == flag_offset(c): fixed for every batch size (mmt_loss_flag_offset)
  p.pack8 = c->fp8 ? A((size_t)c->pack8_bytes) : 0;
  p.act.resize((size_t)c->L * M);
  for (int i = 0; i < M; ++i) p.xemb[i] = A(R * C * f4);
  for (int l = 0; l < c->L; ++l)
    for (int i = 0; i < M; ++i) {
      ActLM& a = p.act[(size_t)l * M + i];
      const LM& x = c->lm[(size_t)l * M + i];
      a.a = A(R * C * b2); a.mean1 = A(R * f4); a.rstd1 = A(R * f4);
      a.h1 = A(R * ldh1 * b2); a.qkv = A(R * 3 * C * b2); a.o = A(R * C * b2); a.lse = A(bhT * f4);
      a.p1 = A(R * ldp * b2); a.x1 = A(R * C * f4);
      a.c = A(R * C * b2); a.mean2 = A(R * f4); a.rstd2 = A(R * f4);
      a.f = A(R * 4 * C * b2); a.x2 = A(R * C * f4);
      a.fm = c->relu_bits ? A(R * (4 * C / 8)) : 0;
      a.x2h = c->any_cross ? A(R * C * b2) : 0;
      a.dm = mbytes ? A(mbytes) : 0;
      if (c->fp8) {
        const int ldsC = (int)rup(C / 32, 4), ldsF = (int)rup(4 * C / 32, 4);
        a.a8 = A(R * C); a.c8 = A(R * C); a.f8 = A(R * 4 * C);
        if (x.cross) a.d8 = A(R * C);
        a.as8 = A(R * ldsC); a.cs8 = A(R * ldsC); a.fs8 = A(R * ldsF);
        if (x.cross) a.ds8 = A(R * ldsC);
      }
      if (x.cross) {
        a.d = A(R * C * b2); a.meanc = A(R * f4); a.rstdc = A(R * f4); a.qc = A(R * C * b2);
        for (int j = 0; j < M - 1; ++j) {
          a.kv[j] = A(R * 2 * C * b2);
          a.ocj[j] = A(R * C * b2);
          a.lsej[j] = A(bhT * f4);
          a.dmj[j] = mbytes ? A(mbytes) : 0;
        }
        a.oc = A(R * C * b2); a.pc = A(R * ldp * b2); a.x3 = A(R * C * f4);
      }
    }
  int maxvh = 8, maxv = 8;
  for (int i = 0; i < M; ++i) { maxvh = std::max(maxvh, c->ldvh[i]); maxv = std::max(maxv, c->ldv[i]); }
  for (int i = 0; i < M; ++i) {
    p.lnf16[i] = A(R * C * b2); p.meanf[i] = A(R * f4); p.rstdf[i] = A(R * f4);
    p.hh[i] = A(R * c->ldvh[i] * b2); p.dlog[i] = A(R * c->ldv[i] * b2);
  }
  for (int i = 0; i < M; ++i) {
    p.dres[i] = A(R * C * f4); p.dln[i] = A(R * C * f4);
    p.eperm[i] = A(R * 4);
    p.celoss[i] = A(512 * 4);
    for (int k = 0; k < 8; ++k) p.dres16[k][i] = A(R * C * b2);
    p.gdo[i] = A(R * C * b2); p.gqkv[i] = A(R * 3 * C * b2);
    for (int k = 0; k < 2; ++k) {
      p.gbig[k][i] = A(R * std::max(4 * C, maxvh) * b2);
      p.gq[k][i] = A(R * C * b2);
      p.gh1[k][i] = A(R * ldh1 * b2); p.gp[k][i] = A(R * ldp * b2);
      p.gpc[k][i] = (c->any_cross && c->cfg.cross_attention[i]) ? A(R * ldp * b2) : p.gp[k][i];
      if (c->any_cross && c->cfg.cross_attention[i])
        for (int j = 0; j < M - 1; ++j) p.dkv[k][i][j] = A(R * 2 * C * b2);
    }
    for (int j = 0; j < M; ++j) p.dvec[i][j] = A(bhT * f4);
  }
  // weight-gradient split-K slabs: room for 16 splits of the largest grouped dW launch
  {
    int64_t mx = 0, heads = 0;
    mx = std::max<int64_t>(mx, (int64_t)M * 4 * C * C);                  // FFN (either matrix)
    mx = std::max<int64_t>(mx, (int64_t)M * r8(3 * H * c->hh) * C);      // Q/K/V stage 1
    mx = std::max<int64_t>(mx, (int64_t)MMT_MAX_GROUP * 2 * C * C);      // cross-attention KV
    for (int i = 0; i < M; ++i) heads += (int64_t)c->V[i] * (c->V[i] / 2 + 4) + (int64_t)(c->V[i] / 2 + 4) * C;
    mx = std::max<int64_t>(mx, heads);
    p.slab_bytes = (size_t)mx * 16 * f4;
    p.slab = A(p.slab_bytes);
  }
  // deterministic mode: the largest partial-sum region any producer launch of the backward needs
  {
    const int Ri = (int)R;
    int64_t df = 0;
    df = std::max(df, mmt_gemm_det_floats(M, Ri, std::max(4 * C, maxvh), false));  // dbias of the data-gradient GEMMs
    df = std::max(df, mmt_gemm_det_floats(M, Ri, C, true));                        // LayerNorm-fused: dsum, dgamma, dbeta
    df = std::max(df, mmt_mlp2_bwd_det_floats(std::min(M, MMT_MLP2_GROUP), Ri, C / 2));
    df = std::max(df, mmt_ln_bwd_det_floats(M, Ri, C));
    df = std::max(df, mmt_colsum_det_floats(M, Ri, maxv));
    df = std::max(df, mmt_drop_copy_det_floats(M, Ri, C));
    df = std::max(df, mmt_qkv2_bwd_det_floats(M, Ri, 3 * H, c->hs));
    if (c->hs == 32) df = std::max(df, mmt_attn_q2_det_floats(M, B, H));
    df = std::max(df, mmt_embed_bwd_det_floats(M, B, c->T, C));
    p.det_floats = df;
    p.det = A((size_t)df * f4);
  }
  // decode scratch (tiny: B rows)
  plan_dec_rows(c, A, (size_t)B, p.dec, p.dec_x, c->L);
  p.total = cur;
}

template <class T>
inline T* at(void* ws, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off); }

// grouped-GEMM helpers ------------------------------------------------------------------------
GemmProblem gp_fwd(const bf16_t* X, int ldx, const bf16_t* Wpk, const Mat& W, int R) {
  GemmProblem g{};
  g.A = X; g.lda = ldx; g.B = Wpk + W.pk; g.ldb = W.ld;
  g.M = R; g.N = W.rows; g.K = W.cols; g.alpha = 1.f;
  return g;
}
// dX = dY W : dY [R, W.rows] (ld ldy), result [R, W.cols]
GemmProblem gp_dx(const bf16_t* dY, int ldy, const bf16_t* Wpk, const Mat& W, int R) {
  GemmProblem g{};
  g.A = dY; g.lda = ldy; g.B = Wpk + W.pk; g.ldb = W.ld;
  g.M = R; g.N = W.cols; g.K = W.rows; g.alpha = 1.f;
  return g;
}
// dW += dY^T X : out [W.rows, W.cols] fp32 in the grad buffer
GemmProblem gp_dw(const bf16_t* dY, int ldy, const bf16_t* X, int ldx, float* grads, const Mat& W, int R) {
  GemmProblem g{};
  g.A = dY; g.lda = ldy; g.B = X; g.ldb = ldx;
  g.M = W.rows; g.N = W.cols; g.K = R; g.o32 = grads + W.off; g.ldc = W.cols; g.alpha = 1.f;
  return g;
}

// live-probe pattern match: "label" exact, "*suffix" (e.g. "*_dw": every weight-gradient GEMM),
// "prefix*"; returns the index of the first matching pattern or -1
int probe_match_one(const mmt_ctx* c, const char* what) {
  const size_t n = std::strlen(what);
  for (size_t i = 0; i < c->probe_pats.size(); ++i) {
    const std::string& p = c->probe_pats[i];
    if (p.empty()) continue;
    if (p[0] == '*') {
      const size_t k = p.size() - 1;
      if (n >= k && std::strcmp(what + n - k, p.c_str() + 1) == 0) return (int)i;
    } else if (p.back() == '*') {
      if (std::strncmp(what, p.c_str(), p.size() - 1) == 0) return (int)i;
    } else if (p == what) {
      return (int)i;
    }
  }
  return -1;
}
// a merged launch is labelled "a+b+...": it matches when any part does
int probe_match(const mmt_ctx* c, const char* what) {
  std::string w(what);
  size_t b = 0;
  while (true) {
    const size_t e = w.find('+', b);
    const int r = probe_match_one(c, w.substr(b, e == std::string::npos ? std::string::npos : e - b).c_str());
    if (r >= 0 || e == std::string::npos) return r;
    b = e + 1;
  }
}

// algorithmic cost of one grouped GEMM launch: 2MNK flops; every operand read once and every
// output written once (bf16 activations / packed bf16 weights, fp32 bias / residual / outputs)
void gemm_cost(const GemmProblem* p, int n, int epi, double* fl, double* by) {
  for (int g = 0; g < n; ++g) {
    const GemmProblem& P = p[g];
    const double M = P.M, N = P.N, K = P.K;
    *fl += 2.0 * M * N * K;
    double x = (M * K + N * K) * 2.0;
    if (P.bias) x += N * 4.0;
    const bool f32_out = epi == EPI_BIAS_RESID_F32 || epi == EPI_STORE_F32 || epi == EPI_ACC_F32;
    x += M * N * (f32_out ? 4.0 : 2.0);
    if (epi == EPI_BIAS_RESID_F32) x += M * N * 4.0 + (P.o16 ? M * N * 2.0 : 0.0);
    if (epi == EPI_ACC_F32) x += M * N * 4.0;
    // tanh' / ReLU' operand: the bf16 hidden rows, or one bit per element (ReLU' bits, mask8)
    if (epi == EPI_DTANH_BF16 || epi == EPI_DRELU_BF16) x += (epi == EPI_DRELU_BF16 && P.mask8) ? M * N / 8.0 : M * N * 2.0;
    // ReLU' bits written by the forward (EPI_BIAS_RELU_BF16 with mask8)
    if (epi == EPI_BIAS_RELU_BF16 && P.mask8) x += M * N / 8.0;
    // MX-fp8 copy of the output (the next fp8 GEMM's A operand): e4m3fn bytes + one E8M0 byte per 32
    if (P.o8) x += M * N * (1.0 + 1.0 / 32.0);
    // fused LayerNorm backward: LN input and the accumulated gradient read, that gradient (+ its bf16
    // copy) written, row statistics read
    if (epi == EPI_LN_BWD_F32) x += M * N * 8.0 + (P.o16 ? M * N * 2.0 : 0.0) + M * 8.0;
    // per-head Q/K/V stage 2 in the epilogue: 2 N output columns written, W2 (fp32 [N / hh][2 hh][hh]) read
    if (P.qkv2_out) {
      x += M * 2.0 * N * 2.0 + 2.0 * N * P.qkv2_hh * 4.0;
      *fl += 2.0 * M * 2.0 * N * P.qkv2_hh;
    }
    *by += x;
  }
}
void gemm_cost(const GemmBatch& b, int epi, double* fl, double* by) { gemm_cost(b.p, b.count, epi, fl, by); }

// weight gradient dW[M,N] += dY[K,M]^T X[K,N]: both operands read once, the fp32 gradient written once
void wgrad_cost(const GemmBatch& b, double* fl, double* by) {
  for (int g = 0; g < b.count; ++g) {
    const GemmProblem& P = b.p[g];
    const double M = P.M, N = P.N, K = P.K;
    *fl += 2.0 * M * N * K;
    *by += (M * K + N * K) * 2.0 + M * N * 4.0;
  }
}

// causal attention, causal-useful count (a = 1/2): per (batch, head, KV stream)
// forward 2 T^2 hs (QK^T and PV over the T(T+1)/2 kept scores), backward 2.5x that (S, dP, dV,
// dQ, dK). Bytes: Q, K, V, O (+ per-stream outputs of a multi-stream problem), log-sum-exp and
// dropout keep bits read / written once; backward adds dO, the row dot products and dQ, dK, dV.
void attn_cost(const AttnBatch& ab, int B, int T, int H, int hs, bool bwd, bool drop, double* fl, double* by) {
  const double C = (double)H * hs, rows = (double)B * T, bhT = (double)B * H * T;
  const double mask = drop ? (double)mmt_attn_mask_dwords(B, H, T) * 4.0 : 0.0;
  for (int g = 0; g < ab.count; ++g) {
    const double ns = ab.p[g].nstreams;
    const double f = 2.0 * (double)B * H * ns * (double)T * T * hs;
    *fl += bwd ? 2.5 * f : f;
    double x = rows * C * 2.0 * (2.0 + 2.0 * ns) + ns * (bhT * 4.0 + mask);  // q, o, k_j, v_j, lse_j, bits
    if (ns > 1) x += ns * rows * C * 2.0;                                      // per-stream outputs o_j
    if (bwd) x += rows * C * 2.0 * (2.0 + 2.0 * ns) + ns * bhT * 4.0;         // dO, dQ, dK_j, dV_j, dvec_j
    if (bwd && ab.p[g].q2_w2) {
      // the stage-2 backward in the epilogue: dQ / dK / dV not written; h1 read, dh1 written (3 H x hs/2
      // columns each), W2 read and dW2 written (algorithmic: once; the kernel adds per workgroup through L2);
      // flops: dh1 = dX W2 and dW2 = dX^T h1
      const double hh = hs / 2;
      x += -rows * C * 2.0 * 3.0 + 2.0 * rows * 3.0 * H * hh * 2.0 + 3.0 * H * hs * hh * 4.0 * 2.0;
      *fl += 2.0 * 2.0 * rows * 3.0 * C * hh;
    }
    if (ab.p[g].oc_w2) {
      // Q / K / V made on chip: their rows are not read; the forward reads h1 and W2 in their place (the
      // backward's epilogue counts both already); flops: X = h1 W2^T
      const double hh = hs / 2;
      x -= rows * C * 2.0 * 3.0;
      if (!bwd) x += rows * 3.0 * H * hh * 2.0 + 3.0 * H * hs * hh * 4.0;
      *fl += 2.0 * rows * 3.0 * C * hh;
    }
    *by += x;
  }
}

// MX-fp8 forward linear: A = e4m3fn activations [R, K] (lda bytes) + exponents, B = the weight's
// MX-fp8 copy in the fp8 pack region
GemmProblem gp_f8(const uint8_t* X8, int ldx, const uint8_t* Xs, int ldxs, const uint8_t* w8, const Mat& W, int R) {
  GemmProblem g{};
  g.A = reinterpret_cast<const bf16_t*>(X8); g.lda = ldx; g.sa = Xs; g.lds_a = ldxs;
  g.B = reinterpret_cast<const bf16_t*>(w8 + W.pk8); g.ldb = W.ld8; g.sb = w8 + W.ps8; g.lds_b = W.lds8;
  g.M = R; g.N = W.rows; g.K = W.cols; g.alpha = 1.f;
  return g;
}

// dropout sites (model.py:69 SA probabilities, :91 SA projection, :151 CA probabilities,
// :116 CA projection, :171 FFN output); one hash key per (seed, layer, modality, site)
enum DropSite { DS_SA_PROB = 0, DS_SA_PROJ = 1, DS_FFN = 2, DS_CA_PROB = 3, DS_CA_PROJ = 4 };

// descriptor builders -------------------------------------------------------------------------
// a batch of n problems, problem u made by fn(u); built where it is launched, so no field of an earlier launch lives on
// (gemms / lns: the two most common kinds)
template <class Bt, class Fn>
Bt batch_of(int n, Fn&& fn) {
  Bt b{};
  b.count = n;
  for (int u = 0; u < n; ++u) b.p[u] = fn(u);
  return b;
}
template <class Fn> GemmBatch gemms(int n, Fn&& fn) { return batch_of<GemmBatch>(n, fn); }
template <class Fn> LnBatch lns(int n, Fn&& fn) { return batch_of<LnBatch>(n, fn); }

// a forward Linear's problem (Runner::linear / linear8) and where its rows go
struct Lin : GemmProblem {
  Lin(const GemmProblem& g) : GemmProblem(g) {}
  Lin& out16(bf16_t* y, int ld) { o16 = y; ldo16 = ld; return *this; }                       // bf16 rows
  Lin& out32(float* y, int ld, const float* res = nullptr) {                                   // fp32 rows (+ residual)
    o32 = y; ldc = ld; resid = res; ldres = res ? ld : 0;
    return *this;
  }
};

LnProblem ln_fwd_problem(const float* x, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd) {
  LnProblem q{};
  q.x = x; q.gamma = gamma; q.beta = beta; q.y = y; q.mean = mean; q.rstd = rstd;
  return q;
}
// dx += the LayerNorm's input gradient; no bf16 copy (set_dres16_consumer / the caller add dx16, dsum and its mask)
LnProblem ln_bwd_problem(const float* x, const float* gamma, float* mean, float* rstd, const float* dy, float* dx,
                         float* dgamma, float* dbeta) {
  LnProblem q{};
  q.x = x; q.gamma = gamma; q.mean = mean; q.rstd = rstd;
  q.dy = dy; q.dx = dx; q.dgamma = dgamma; q.dbeta = dbeta;
  return q;
}
// the three LayerNorms of a layer: where each keeps its parameters (LM) and its saved rows (ActLM)
struct LnSite {
  int64_t LM::*w, LM::*b;
  size_t ActLM::*y, ActLM::*mean, ActLM::*rstd, ActLM::*y8, ActLM::*s8;
};
const LnSite LN1{&LM::ln1w, &LM::ln1b, &ActLM::a, &ActLM::mean1, &ActLM::rstd1, &ActLM::a8, &ActLM::as8};
const LnSite LN2{&LM::ln2w, &LM::ln2b, &ActLM::c, &ActLM::mean2, &ActLM::rstd2, &ActLM::c8, &ActLM::cs8};
const LnSite LNC{&LM::lncw, &LM::lncb, &ActLM::d, &ActLM::meanc, &ActLM::rstdc, &ActLM::d8, &ActLM::ds8};
// the LayerNorm n in the epilogue of the residual GEMM that writes its input rows (GemmProblem::lnf_*)
void fuse_next_ln(GemmProblem& g, const LnProblem& n) {
  g.lnf_gamma = n.gamma; g.lnf_beta = n.beta; g.lnf_y = n.y; g.lnf_mean = n.mean; g.lnf_rstd = n.rstd;
}

// the operand fields AttnProblem, DecodeAttnProblem and FanoutAttnProblem share. Self-attention: K | Q | V
// interleaved in rows of 3C (kqv), the query row given apart (decode reads it from compact or tail rows)
template <class P>
void self_attn_io(P& q, const bf16_t* qrow, int q_ld, const bf16_t* kqv, bf16_t* o, int C, int hs) {
  q.q = qrow; q.q_ld = q_ld; q.k[0] = kqv; q.v[0] = kqv + 2 * C; q.kv_ld = 3 * C; q.kv_hstride = hs;
  q.o = o; q.o_ld = C; q.nstreams = 1;
}
// cross-attention over nkv KV streams, stream j's K | V interleaved per head in the rows of 2C that kv(j) returns
template <class P, class Kv>
void cross_attn_io(P& q, const bf16_t* qrow, Kv&& kv, int nkv, bf16_t* o, int C, int hs) {
  q.q = qrow; q.q_ld = C;
  for (int j = 0; j < nkv; ++j) { q.k[j] = kv(j); q.v[j] = q.k[j] + hs; }
  q.kv_ld = 2 * C; q.kv_hstride = 2 * hs; q.o = o; q.o_ld = C; q.nstreams = nkv;
}

inline std::vector<int> cross_set(const LM* x, int M) {
  std::vector<int> cx;
  for (int i = 0; i < M; ++i) if (x[i].cross) cx.push_back(i);
  return cx;
}
// the cross K/V projections of a layer: for every cross modality i of cx and every other modality j (i's KV stream
// jj), add(i, j, jj) appends one problem to the caller's group and send() launches and empties it: at MMT_MAX_GROUP
// problems, at the end, and (per_query) after each i's last stream
template <class Add, class Send>
void for_each_cross_kv(const std::vector<int>& cx, int M, bool per_query, Add&& add, Send&& send) {
  int n = 0;
  for (int i : cx) {
    int jj = 0;
    for (int j = 0; j < M; ++j) {
      if (j == i) continue;
      add(i, j, jj++);
      if (++n == MMT_MAX_GROUP) { send(); n = 0; }
    }
    if (per_query && n) { send(); n = 0; }
  }
  if (n) send();
}

struct Runner {
  mmt_ctx* c;
  hipStream_t s;
  void* ws;
  const float* params;
  const bf16_t* wpk;
  int B, R;
  int rc = MMT_OK;
  bool drop = false;  // dropout active for this forward / its backward
  uint64_t seed = 0;

  template <class T> T* W(size_t off) { return at<T>(ws, off); }
  bf16_t* b16(size_t off) { return at<bf16_t>(ws, off); }
  float* f32(size_t off) { return at<float>(ws, off); }
  const float* P(int64_t off) { return params + off; }

  // element kept iff mmt_keep(mmt_hash(key, row, col >> 1), col, thr) ; kept values scaled by 1 / (1 - p)
  template <class Pm>
  void set_drop(Pm& p, int l, int i, int site) const {
    if (!drop) { p.drop_key = 0; p.drop_thr = 0; p.drop_scale = 1.f; return; }
    const double pr = c->cfg.dropout;
    p.drop_key = mmt_hash((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)((l * MAXM + i) * 8 + site));
    p.drop_thr = (uint32_t)std::min(65535.0, std::max(1.0, std::floor(pr * 65536.0)));  // 16-bit halves (mmt_keep)
    p.drop_scale = (float)(1.0 / (1.0 - pr));
  }

  // Y = X W^T (+ bias; bias < 0: none) on bf16 rows X [R, W.cols] against the packed bf16 weight
  Lin linear(const bf16_t* X, int ldx, const Mat& W, int64_t bias) {
    GemmProblem g = gp_fwd(X, ldx, wpk, W, R);
    if (bias >= 0) g.bias = P(bias);
    return g;
  }
  // the same on the MX-fp8 copies of X and W (precision fp8)
  Lin linear8(const uint8_t* X8, int ldx, const uint8_t* Xs, int ldxs, const uint8_t* w8, const Mat& W, int64_t bias) {
    GemmProblem g = gp_f8(X8, ldx, Xs, ldxs, w8, W, R);
    if (bias >= 0) g.bias = P(bias);
    return g;
  }
  // the training forward's and backward's self-attention problem of (layer l, modality i): the fields both share
  AttnProblem self_attn(const ActLM& a, int l, int i) {
    AttnProblem q{};
    bf16_t* kqv = b16(a.qkv);
    self_attn_io(q, kqv + c->C, 3 * c->C, kqv, b16(a.o), c->C, c->hs);
    q.lse[0] = f32(a.lse);
    set_drop(q, l, i, DS_SA_PROB);
    if (drop) q.dmask[0] = W<uint32_t>(a.dm);
    return q;
  }
  // ... and the cross-attention problem of a cross modality i over the other M - 1 modalities' K/V
  AttnProblem cross_attn(const ActLM& a, int l, int i) {
    AttnProblem q{};
    const int nkv = c->M - 1;
    cross_attn_io(q, b16(a.qc), [&](int j) { return b16(a.kv[j]); }, nkv, b16(a.oc), c->C, c->hs);
    for (int j = 0; j < nkv; ++j) { q.oj[j] = b16(a.ocj[j]); q.lse[j] = f32(a.lsej[j]); }
    set_drop(q, l, i, DS_CA_PROB);
    if (drop)
      for (int j = 0; j < nkv; ++j) q.dmask[j] = W<uint32_t>(a.dmj[j]);
    return q;
  }

  bool ok(hipError_t e, const char* what) {
    if (e != hipSuccess && rc == MMT_OK) rc = fail(c, MMT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return e == hipSuccess;
  }
  // deterministic mode (backward only): hands a producer launch the partial-sum scratch; its ordered sum is
  // launched by the producer's launcher right behind it, between the probe hooks (label "det_sum")
  bool det = false;
  int det_probe = -1;
  static void det_hook(void* user, int after) {
    Runner* r = static_cast<Runner*>(user);
    if (!after) r->det_probe = r->probe_begin("det_sum", r->s);
    else r->probe_end(r->det_probe, r->s, 0.0, 0.0);
  }
  template <class Bt>
  void det_arm(Bt& b) {
    if (!det) return;
    b.det.base = W<float>(c->plan.det);
    b.det.cap = c->plan.det_floats;
    b.det.stride = 0;
    b.det.hook = &Runner::det_hook;
    b.det.user = this;
  }
  // live kernel timing (mmt_probe_set): HIP events around every launch whose label matches one of
  // the probe patterns, recorded on the stream the launch goes to (the side stream for weight
  // gradients), each tagged with the launch's algorithmic flops and bytes
  int probe_begin(const char* what, hipStream_t st) {
    if (!c->probe_on || c->probe_pats.empty()) return -1;
    const int pat = probe_match(c, what);
    if (pat < 0) return -1;
    if (c->probe_events.size() >= c->probe_pool.size()) return -1;  // pool exhausted: stop recording
    mmt_ctx::ProbeEv e{};
    e.a = c->probe_pool[c->probe_events.size()].first;
    e.b = c->probe_pool[c->probe_events.size()].second;
    e.pat = pat;
    hipEventRecord(e.a, st);
    c->probe_events.push_back(e);
    return (int)c->probe_events.size() - 1;
  }
  void probe_end(int id, hipStream_t st, double flops, double bytes) {
    if (id < 0) return;
    mmt_ctx::ProbeEv& e = c->probe_events[id];
    e.flops = flops;
    e.bytes = bytes;
    hipEventRecord(e.b, st);
  }
  // Every labelled launch goes through here: the error latch (after a failure nothing more is launched), the probe
  // events around go() on the stream it launches to, and, only when a pattern matched, cost(&flops, &bytes)
  template <class Go, class Cost>
  void launch(const char* what, hipStream_t st, Go&& go, Cost&& cost) {
    if (rc != MMT_OK) return;
    const int id = probe_begin(what, st);
    ok(go(), what);
    if (id < 0) return;
    double fl = 0, by = 0;
    cost(&fl, &by);
    probe_end(id, st, fl, by);
  }
  // GemmBatch::tile_hint for the main-stream GEMMs launched while it is set (run_forward: beside the
  // side stream's keep-bit launches)
  int gemm_hint = 0;
  static void set_hint(GemmBatch& b, int hint) { b.tile_hint = hint; }
  static void set_hint(AttnBatch&, int) {}
  // go(the batch as launched): b itself, or a copy that carries the tile hint and (arm, deterministic mode) the
  // partial-sum scratch
  template <class Bt, class Go>
  hipError_t prepared(const Bt& b, int hint, bool arm, Go&& go) {
    if (!hint && !(arm && det)) return go(b);
    Bt h = b;
    if (hint) set_hint(h, hint);
    if (arm) det_arm(h);
    return go(h);
  }
  void gemm(const GemmBatch& b, bool akc, bool bkc, int epi, int splits, const char* what) {
    auto go = [&](const GemmBatch& h) { return mmt_launch_gemm(h, akc, bkc, epi, splits, s); };
    launch(what, s, [&] { return prepared(b, gemm_hint, true, go); }, [&](double* fl, double* by) { gemm_cost(b, epi, fl, by); });
  }
  // MX-fp8 forward GEMM (precision fp8): A / B e4m3fn + E8M0 (mmt_launch_gemm_f8)
  void gemm8(const GemmBatch& b, int epi, const char* what) {
    auto go = [&](const GemmBatch& h) { return mmt_launch_gemm_f8(h, epi, s); };
    launch(what, s, [&] { return prepared(b, gemm_hint, false, go); },
           [&](double* fl, double* by) {
             gemm_cost(b, epi, fl, by);
             // 1-byte operands plus one E8M0 exponent byte per 32 K elements of every row of A and B
             for (int g = 0; g < b.count; ++g) *by -= ((double)b.p[g].M + b.p[g].N) * b.p[g].K * (1.0 - 1.0 / 32.0);
           });
  }
  // a forward Linear launch (both operands K-contiguous, no split): the MX-fp8 kernel when f8
  void fgemm(const GemmBatch& b, int epi, const char* what, bool f8 = false) {
    if (f8) gemm8(b, epi, what);
    else gemm(b, true, true, epi, 1, what);
  }
  // backward-data GEMM dy = A B (EPI_STORE_F32 into lb's dy) followed by the LayerNorm backward lb
  // (model.py:189-190, 210, 330 under autograd): ONE launch with the LayerNorm fused into the GEMM's
  // epilogue when every problem's rows fit one tile (C == 256 or 512; MMT_LN_FUSE=0 disables), else
  // the two passes. The fused launch never materialises dy (the fp32 round trip of the two-pass form)
  void gemm_ln_bwd(const GemmBatch& dx, const LnBatch& lb, int R, int C, const char* gname, const char* lname) {
    if (rc != MMT_OK) return;
    if (knobs().ln_fuse != 0 && lb.count == dx.count) {
      GemmBatch f = dx;
      for (int g = 0; g < f.count; ++g) {
        GemmProblem& P = f.p[g];
        const LnProblem& Lp = lb.p[g];
        P.o32 = Lp.dx; P.ldc = C;
        P.resid = Lp.x; P.ldres = C;
        P.ln_gamma = Lp.gamma; P.ln_mean = Lp.mean; P.ln_rstd = Lp.rstd;
        P.ln_dgamma = Lp.dgamma; P.ln_dbeta = Lp.dbeta;
        P.o16 = Lp.dx16; P.ldo16 = C; P.dbias = Lp.dsum;
        P.drop_key = Lp.drop_key; P.drop_thr = Lp.drop_thr; P.drop_scale = Lp.drop_scale;
        P.bias = nullptr; P.aux = nullptr; P.split_stride = 0;
      }
      if (mmt_gemm_ln_bwd_ok(f)) {
        det_arm(f);
        launch(gname, s, [&] { return mmt_launch_gemm_ln_bwd(f, s); },
               [&](double* fl, double* by) { gemm_cost(f, EPI_LN_BWD_F32, fl, by); });
        return;
      }
    }
    gemm(dx, true, false, EPI_STORE_F32, 1, gname);
    LnBatch ld = lb;
    det_arm(ld);
    ok(mmt_launch_ln_bwd(ld, R, C, s), lname);
  }
  // n problem pairs (g1s[i] feeds g2s[i] through a hidden tile that stays on chip) as Mlp2Batch chunks of
  // MMT_MLP2_GROUP under ONE label: nothing is launched and false returned unless fits() takes every chunk.
  // Cost: the two GEMMs' (epilogues epi1, epi2), less the hidden rows the second product does not read back
  template <class Fits, class Go>
  bool pair_launch(const GemmProblem* g1s, const GemmProblem* g2s, int n, const char* what, int epi1, int epi2, bool arm,
                   Fits&& fits, Go&& go) {
    Mlp2Batch chunk[(MMT_MAX_GROUP + MMT_MLP2_GROUP - 1) / MMT_MLP2_GROUP] = {};
    const int nch = (n + MMT_MLP2_GROUP - 1) / MMT_MLP2_GROUP;
    for (int i = 0; i < n; ++i) {
      Mlp2Batch& b = chunk[i / MMT_MLP2_GROUP];
      b.g1[b.count] = g1s[i];
      b.g2[b.count] = g2s[i];
      ++b.count;
    }
    for (int k = 0; k < nch; ++k)
      if (!fits(chunk[k])) return false;
    if (arm)
      for (int k = 0; k < nch; ++k) det_arm(chunk[k]);  // (each chunk's ordered sum runs before the next chunk's launch)
    launch(what, s,
           [&] {
             hipError_t first = hipSuccess;
             for (int k = 0; k < nch; ++k) {
               const hipError_t e = go(chunk[k], s);
               if (first == hipSuccess) first = e;
             }
             return first;
           },
           [&](double* fl, double* by) {
             gemm_cost(g1s, n, epi1, fl, by);
             gemm_cost(g2s, n, epi2, fl, by);
             for (int g = 0; g < n; ++g) *by -= (double)g2s[g].M * g2s[g].K * 2.0;  // h / dh is not read back
           });
    return true;
  }
  // the attention out-projection Linear(C, C/2) -> tanh -> Linear(C/2, C) + dropout + residual as one fused
  // launch (mmt_launch_mlp2: h stays in LDS between the products); false (nothing launched) when the
  // shape is outside the fused kernel or MMT_MLP2=0, and the caller runs the two GEMMs
  // bwd: the backward-data pair (mmt_launch_mlp2_bwd: dh = (dY W2) tanh', dx = dh W0), by MMT_MLP2_BWD
  bool mlp2(const GemmProblem* g1s, const GemmProblem* g2s, int n, const char* what, bool bwd = false) {
    const int bwd_mode = knobs().mlp2_bwd;
    const bool on_bwd = bwd_mode == 1 || (bwd_mode == 2 && n >= 1 && g1s[0].N == 128);
    if (rc != MMT_OK || knobs().mlp2 == 0 || (bwd && !on_bwd) || n < 1) return false;
    if (bwd) return pair_launch(g1s, g2s, n, what, EPI_DTANH_BF16, EPI_STORE_BF16, true, mmt_mlp2_bwd_ok, mmt_launch_mlp2_bwd);
    return pair_launch(g1s, g2s, n, what, EPI_BIAS_TANH_BF16, EPI_BIAS_RESID_F32, false, mmt_mlp2_ok, mmt_launch_mlp2);
  }
  // the FFN forward Linear(C, 4C) -> ReLU -> Linear(4C, C) + dropout + residual (+ the next LayerNorm) as one
  // launch (mmt_launch_ffn: the hidden activation is stored for the backward but never read back); g1s the
  // ffn0 problems, g2s the ffn2 problems. false (nothing launched) when the shape is outside the kernel
  bool ffn(const GemmProblem* g1s, const GemmProblem* g2s, int n, const char* what) {
    if (rc != MMT_OK || n < 1) return false;
    return pair_launch(g1s, g2s, n, what, EPI_BIAS_RELU_BF16, EPI_BIAS_RESID_F32, false, mmt_ffn_ok, mmt_launch_ffn);
  }
  // forward residual GEMM with the next LayerNorm's forward fused (mmt_launch_gemm_resid_ln)
  bool gemm_resid_ln(const GemmBatch& b, const char* what) {
    if (rc != MMT_OK || !mmt_gemm_resid_ln_ok(b)) return false;
    launch(what, s, [&] { return mmt_launch_gemm_resid_ln(b, s); },
           [&](double* fl, double* by) {
             gemm_cost(b, EPI_BIAS_RESID_F32, fl, by);
             for (int g = 0; g < b.count; ++g)
               if (b.p[g].lnf_y) *by += (double)b.p[g].M * b.p[g].N * 2.0 + b.p[g].M * 8.0;
           });
    return true;
  }
  void attn(const AttnBatch& ab, bool bwd, float scale, const char* what) {
    const auto kernel = bwd ? mmt_launch_attn_bwd : mmt_launch_attn_fwd;
    auto go = [&](const AttnBatch& h) { return kernel(h, B, c->T, c->H, c->hs, scale, s); };
    launch(what, s, [&] { return prepared(ab, 0, bwd, go); },
           [&](double* fl, double* by) { attn_cost(ab, B, c->T, c->H, c->hs, bwd, drop, fl, by); });
  }
  // fork the side stream off the main one (everything enqueued on `s` so far happens first)
  hipStream_t side_stream() const { return c->side_off ? nullptr : c->side; }
  hipStream_t side() {
    if (!side_stream()) return s;
    hipEvent_t e = c->evpool[c->evnext++ % c->evpool.size()];
    ok(hipEventRecord(e, s), "event record");
    ok(hipStreamWaitEvent(c->side, e, 0), "stream wait");
    return c->side;
  }
  // the main stream waits for everything enqueued on the side stream
  void join() {
    flush(true);
    if (!side_stream()) return;
    hipEvent_t e = c->evpool[c->evnext++ % c->evpool.size()];
    ok(hipEventRecord(e, c->side), "event record");
    ok(hipStreamWaitEvent(s, e, 0), "stream wait");
  }
  // weight-gradient GEMMs go to the side stream in batches: dwgemm() queues one, flush() forks the
  // side stream once (after everything its queued GEMMs read is enqueued on the main stream) and
  // launches them. Every fork / join is a barrier packet costing ~10 us of main-stream idle, so
  // the stage code flushes a few times per layer instead of forking per GEMM.
  std::vector<std::pair<GemmBatch, const char*>> pend;
  // hold: the stage's intermediate flushes keep their launches queued for the stage-end flush (one fork
  // per stage instead of one per flush point; each fork's event record costs the main stream a gap)
  bool hold = false;
  void flush(bool force = false) {
    if (hold && !force && rc == MMT_OK) return;
    if (pend.empty() || rc != MMT_OK) { pend.clear(); return; }
    hipStream_t ss = side_stream() ? side() : s;
    // merge consecutive queued weight-gradient batches of the same tile kind into one launch (up
    // to MMT_MAX_GROUP problems): more tiles per launch -> fewer K splits -> fewer partial bytes
    std::vector<std::pair<GemmBatch, std::string>> merged;
    for (auto& q : pend) {
      if (!merged.empty()) {
        GemmBatch& m = merged.back().first;
        if (m.count + q.first.count <= MMT_MAX_GROUP && wgrad_small(m) == wgrad_small(q.first)) {
          for (int g = 0; g < q.first.count; ++g) m.p[m.count++] = q.first.p[g];
          merged.back().second += std::string("+") + q.second;
          continue;
        }
      }
      merged.emplace_back(q.first, q.second);
    }
    for (auto& q : merged) wgrad(q.first, q.second.c_str(), ss);
    pend.clear();
  }
  // whether a weight-gradient batch stays on the 128 x 128 tile (launches can only be merged when equal)
  static bool wgrad_small(const GemmBatch& b) {
    return mmt_gemm_plan(b, GEMM_WGRAD).tile == GEMM_TILE_128;
  }
  void wgrad(const GemmBatch& b, const char* what, hipStream_t st) {
    launch(what, st, [&] { return mmt_launch_gemm_wgrad(b, W<float>(c->plan.slab), (int64_t)c->plan.slab_bytes, st); },
           [&](double* fl, double* by) { wgrad_cost(b, fl, by); });
  }
  // weight-gradient GEMMs share one split-K slab region: they run in launch order on ONE stream
  // (the side stream when there is one), so no two of them ever write the slabs at once (a
  // probed launch no longer jumps to the main stream: ADVICE r1)
  void dwgemm(const GemmBatch& b, const char* what, int hint = 0) {
    if (rc != MMT_OK) return;
    pend.emplace_back(b, what);  // launched (merged) at the next flush(), on the side stream if any
    pend.back().first.tile_hint = hint;
    // hs 64 (the two-pass attention backward beside them): 96 blocks per launch leave it more CUs. Same box,
    // two passes: C3 142.6-142.9 -> 141.0-141.2 ms (its attention backward 1244 -> 1038 us live), target
    // 19.36-19.40 -> 19.28-19.31, C4 equal; at hs 32 (C1) 96 measured equal to 128 on one box, +0.2 % on
    // another (profiles/r6ak_wgrad_blocks_ab.txt, r6al_wgrad96_ab.txt). MMT_WGRAD_BLOCKS overrides both
    pend.back().first.dw_blocks = c->hs >= 64 ? 96 : 0;
  }
};

// -------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------
// post block (model.py:296-330), shared by the forward and the decode step: the final LayerNorm of the modalities
// lnf_done does not mark (the ffn2 epilogue did theirs), Linear(C, V/2) + tanh, Linear(V/2, V) into logits. rows(i)
// says where modality i's rows live; lf arrives empty but for the words its launch zeroes; labels: lnf, head0, head2
struct PostRows { bf16_t* y; float* mean; float* rstd; bf16_t* hh; };
template <class Rows>
void run_post(mmt_ctx* c, Runner& r, int R, const std::vector<const float*>& xin, const char* lnf_done, Rows&& rows,
              float* const* logits, LnBatch lf, const char* const (&labels)[3]) {
  const int M = c->M, C = c->C;
  for (int i = 0; i < M; ++i) {
    if (lnf_done && lnf_done[i]) continue;
    const PostRows w = rows(i);
    lf.p[lf.count++] = ln_fwd_problem(xin[i], r.P(c->post[i].lnw), r.P(c->post[i].lnb), w.y, w.mean, w.rstd);
  }
  if (lf.count) {
    r.ok(mmt_launch_ln_fwd(lf, R, C, r.s), labels[0]);
  } else if (lf.nzero_f) {  // every post-block LayerNorm was fused: zero the accumulators here
    r.ok(hipMemsetAsync(lf.zero_f, 0, sizeof(float) * lf.nzero_f, r.s), "memset losses");
    r.ok(hipMemsetAsync(lf.zero_i, 0, sizeof(int) * lf.nzero_i, r.s), "memset flag");
  }
  r.fgemm(gemms(M, [&](int i) {
            return r.linear(rows(i).y, C, c->post[i].H0, c->post[i].b0).out16(rows(i).hh, c->ldvh[i]);
          }), EPI_BIAS_TANH_BF16, labels[1]);
  r.fgemm(gemms(M, [&](int i) {
            return r.linear(rows(i).hh, c->ldvh[i], c->post[i].H2, c->post[i].b2).out32(logits[i], c->V[i]);
          }), EPI_STORE_F32, labels[2]);
}

int run_forward(mmt_ctx* c, Runner& r, const int64_t* const* idx, const int64_t* const* tgt, float* const* logits,
                float* losses) {
  const int M = c->M, C = c->C, H = c->H, hs = c->hs, R = r.R, B = r.B, T = c->T;
  const int ldh1 = r8(3 * H * c->hh), ldp = r8(C / 2);
  const float scale = 1.0f / std::sqrt((float)hs);
  const Knobs& kn = knobs();
  Plan& p = c->plan;
  bf16_t* wpk = r.b16(p.pack);
  r.wpk = wpk;
  // keep bits of layer ll's self- and cross-attention dropout, one side-stream launch each (the
  // mask kernel reads nothing the main stream writes: a fork orders it after the previous step)
  hipStream_t ss = r.s;
  const int ahead_mode = kn.mask_ahead >= 0 ? kn.mask_ahead : (c->L >= 12 ? 1 : 0);  // (Knobs: MMT_MASK_AHEAD)
  const bool mask_ahead = ahead_mode != 0;
  auto gen_masks = [&](int ll) {
    if (ll <= 1 || mask_ahead) ss = r.side();  // layer 0: one fork; layers 1..L-1: one fork for all
    const LM* xl = &c->lm[(size_t)ll * M];
    const ActLM* al = &p.act[(size_t)ll * M];
    AttnBatch mb{}; mb.count = M;
    for (int i = 0; i < M; ++i) {
      r.set_drop(mb.p[i], ll, i, DS_SA_PROB);
      mb.p[i].nstreams = 1; mb.p[i].dmask[0] = r.W<uint32_t>(al[i].dm);
    }
    r.ok(mmt_launch_attn_mask(mb, B, T, H, ss), "attn_mask");
    if (!c->any_cross) return;
    AttnBatch mc{}; mc.count = 0;
    for (int i = 0; i < M; ++i) {
      if (!xl[i].cross) continue;
      AttnProblem& q = mc.p[mc.count++];
      r.set_drop(q, ll, i, DS_CA_PROB);
      q.nstreams = M - 1;
      for (int j = 0; j < M - 1; ++j) q.dmask[j] = r.W<uint32_t>(al[i].dmj[j]);
    }
    if (mc.count) r.ok(mmt_launch_attn_mask(mc, B, T, H, ss), "ca_attn_mask");
  };
  if (!r.ok(mmt_launch_pack(c->d_segs, (int)c->segs.size(), (int64_t)c->tasks.size() / 2, c->d_tasks, r.params, wpk,
                            r.s), "pack"))
    return r.rc;
  const bool f8 = c->fp8;
  uint8_t* w8 = f8 ? r.W<uint8_t>(p.pack8) : nullptr;
  const int ldsC = (int)rup(C / 32, 4), ldsF = (int)rup(4 * C / 32, 4);
  if (f8) {
    r.ok(mmt_launch_mx_quant(c->d_mxsegs, (int)c->mxsegs.size(), c->mx_units, r.params, w8, r.s), "mx_quant");
    if ((C / 32) % 4) {  // exponent bytes past C/32 of a row: finite (127) for the K-step that straddles C
      for (int l = 0; l < c->L; ++l)
        for (int i = 0; i < M; ++i) {
          const ActLM& a = p.act[(size_t)l * M + i];
          r.ok(hipMemsetAsync(r.W<uint8_t>(a.as8), 127, (size_t)R * ldsC, r.s), "memset exps");
          r.ok(hipMemsetAsync(r.W<uint8_t>(a.cs8), 127, (size_t)R * ldsC, r.s), "memset exps");
          if (c->lm[(size_t)l * M + i].cross) r.ok(hipMemsetAsync(r.W<uint8_t>(a.ds8), 127, (size_t)R * ldsC, r.s), "memset exps");
        }
    }
  }
  // a Linear of the layers on the rows at x16: on their MX-fp8 copy (x8, exponents s8 with row stride lds) when fp8
  auto lin = [&](size_t x16, size_t x8, size_t s8, int K, int lds, const Mat& W, int64_t bias) {
    return f8 ? r.linear8(r.W<uint8_t>(x8), K, r.W<uint8_t>(s8), lds, w8, W, bias) : r.linear(r.b16(x16), K, W, bias);
  };
  // the LayerNorms, as their own launch reads them (x: the input rows) or as a residual GEMM's epilogue takes them
  // (fuse_next_ln; x unused). fp8: the launch also writes the MX-fp8 copy of y
  auto ln = [&](const LnSite& n, int l, int i, const float* xi) {
    const LM& x = c->lm[(size_t)l * M + i];
    const ActLM& a = p.act[(size_t)l * M + i];
    LnProblem q = ln_fwd_problem(xi, r.P(x.*n.w), r.P(x.*n.b), r.b16(a.*n.y), r.f32(a.*n.mean), r.f32(a.*n.rstd));
    if (f8) { q.y8 = r.W<uint8_t>(a.*n.y8); q.s8 = r.W<uint8_t>(a.*n.s8); q.ld8 = C; q.lds8 = ldsC; }
    return q;
  };
  auto post_rows = [&](int i) { return PostRows{r.b16(p.lnf16[i]), r.f32(p.meanf[i]), r.f32(p.rstdf[i]), r.b16(p.hh[i])}; };
  {
    EmbBatch eb{};
    eb.count = M;
    for (int i = 0; i < M; ++i) {
      eb.p[i].idx = idx[i]; eb.p[i].tok = r.P(c->post[i].tok); eb.p[i].pos = r.P(c->pos_off);
      eb.p[i].x = r.f32(p.xemb[i]); eb.p[i].V = c->V[i];
    }
    r.ok(mmt_launch_embed_fwd(eb, B, T, C, r.s), "embed_fwd");
  }
  std::vector<const float*> xin(M);
  for (int i = 0; i < M; ++i) xin[i] = r.f32(p.xemb[i]);
  // LayerNorm forwards done by the previous residual GEMM's epilogue (Knobs: MMT_LN_FUSE, MMT_LN_FUSE_FWD)
  const int ln_fuse = kn.ln_fuse != 0 ? kn.ln_fuse_fwd : 0;
  const bool fuse_fwd = ln_fuse && !f8 && (C == 256 || (C == 512 && ln_fuse == 2));
  std::vector<char> ln1_done(M, 0), lnf_done(M, 0);
  for (int l = 0; l < c->L && r.rc == MMT_OK; ++l) {
    const LM* x = &c->lm[(size_t)l * M];
    const ActLM* a = &p.act[(size_t)l * M];
    // attention dropout keep bits: layer 0's made on the side stream while the first LayerNorm and
    // Q/K/V GEMMs run, all later layers' while layer 0 computes (two forks, two joins per forward)
    if (r.drop && l == 0) gen_masks(0);
    {
      LnBatch lb{};
      for (int i = 0; i < M; ++i)
        if (!ln1_done[i]) lb.p[lb.count++] = ln(LN1, l, i, xin[i]);
      if (lb.count) r.ok(mmt_launch_ln_fwd(lb, R, C, r.s), "ln1_fwd");
      std::fill(ln1_done.begin(), ln1_done.end(), 0);
    }
    // Q/K/V stage 1; the per-head stage 2 in its epilogue at hs 32 / 64 (Knobs: MMT_QKV2_FUSE), else its own launch
    GemmBatch qkv1 = gemms(M, [&](int i) {
      return lin(a[i].a, a[i].a8, a[i].as8, C, ldsC, x[i].W1, x[i].b1).out16(r.b16(a[i].h1), ldh1);
    });
    // (the 128 x 128 bf16 tile only: not on the fp8 kernel, not where the launch below leaves that tile)
    const bool fuse_qkv2 = kn.qkv2_fuse != 0 && (c->hh == 16 || c->hh == 32) && !f8 &&
                           mmt_gemm_plan(qkv1, GEMM_LINEAR, true, true, EPI_BIAS_TANH_BF16, 1, 0).tile == GEMM_TILE_128;
    AttnBatch ab = batch_of<AttnBatch>(M, [&](int i) { return r.self_attn(a[i], l, i); });
    // Q / K / V on chip (mmt_set_attn_qkv_onchip; training forwards only): exactly where this GEMM would make
    // them in its epilogue and the backward will take the one-pass hs-32 kernel with the stage-2 backward in it.
    // Bit 0: the attention forward makes them from h1 and W2; bit 1: the backward will; both: stage 2 leaves this
    // GEMM and the rows are never written. The same for every layer, kept in c->onchip for the backward.
    int oc = 0;
    if (c->onchip_req && fuse_qkv2 && kn.attn_qkv2 && mmt_attn_bwd_fuses_qkv2(ab, B, T, H, hs) && !(ldh1 & 7)) {
      oc = c->onchip_req;
      for (int i = 0; i < M; ++i)
        if (((uintptr_t)r.b16(a[i].h1) | (uintptr_t)r.P(x[i].w2)) & 15) oc = 0;
    }
    if (l == 0) c->onchip = oc;
    else if (oc != c->onchip) {
      r.rc = fail(c, MMT_ERR_STATE, "mmt_forward: the layers disagree on the on-chip Q/K/V path");
      break;
    }
    for (int i = 0; i < M; ++i) {
      GemmProblem& g = qkv1.p[i];
      if (fuse_qkv2 && oc != 3) {
        g.qkv2_w2 = r.P(x[i].w2); g.qkv2_out = r.b16(a[i].qkv); g.qkv2_ld = 3 * C; g.qkv2_hh = c->hh;
      }
      // both bits: no stage 2 and no Q/K/V store, but h1 bit for bit as the fused launch rounds it
      if (oc == 3) g.qkv2_h1_only = 1;
      if (oc & 1) { ab.p[i].oc_h1 = r.b16(a[i].h1); ab.p[i].oc_ld = ldh1; ab.p[i].oc_w2 = r.P(x[i].w2); }
    }
    r.fgemm(qkv1, EPI_BIAS_TANH_BF16, "qkv1", f8);
    if (!fuse_qkv2) {
      Qkv2Batch qb{}; qb.count = M;
      for (int i = 0; i < M; ++i) {
        qb.p[i].h1 = r.b16(a[i].h1); qb.p[i].w2 = r.P(x[i].w2); qb.p[i].out = r.b16(a[i].qkv);
      }
      r.ok(mmt_launch_qkv2_fwd(qb, R, 3 * H, hs, ldh1, 3 * C, r.s), "qkv2_fwd");
    }
    if (r.drop && (l <= 1 || mask_ahead)) {
      r.join();  // this layer's keep bits (SA and CA) are in (layer 1: every later layer's too)
      r.gemm_hint = 0;
      if (mask_ahead) {
        if (ahead_mode == 1 && l + 1 < c->L) gen_masks(l + 1);
      } else if (l == 0) {
        for (int ll = 1; ll < c->L; ++ll) gen_masks(ll);
        // until layer 1's join the later layers' keep bits fill the CUs the side stream can reach: a
        // ping-pong GEMM block needs a CU with none of them on it (all its VGPRs and 128 KiB of LDS), the
        // 128 x 256 tile fits beside them (Knobs: MMT_MASK_T2)
        if (kn.mask_t2) r.gemm_hint = 1;
      }
    }
    r.attn(ab, false, scale, "attn_fwd");
    if (r.drop && ahead_mode == 2 && l + 1 < c->L) {
      gen_masks(l + 1);
      if (kn.mask_t2) r.gemm_hint = 1;
    }
    // out-projection: Linear(C, C/2) -> tanh -> Linear(C/2, C) -> dropout -> + residual (model.py:82-92,
    // 224), fused into one launch where the shape allows (C = 256 / 512), else two GEMMs. The fused launch owns
    // whole rows: ln2 runs in its epilogue (Knobs: MMT_LN2_FUSE; not fp8, whose ln2 pass also writes the MX copy)
    const bool ln2_fuse = kn.ln2_fuse != 0 && !f8;
    bool ln2_done = false;
    {
      GemmBatch p0 = gemms(M, [&](int i) {
        return r.linear(r.b16(a[i].o), C, x[i].P0, x[i].bp0).out16(r.b16(a[i].p1), ldp);
      });
      GemmBatch p2 = gemms(M, [&](int i) {
        Lin g = r.linear(r.b16(a[i].p1), ldp, x[i].P2, x[i].bp2).out32(r.f32(a[i].x1), C, xin[i]);
        r.set_drop(g, l, i, DS_SA_PROJ);
        if (ln2_fuse) fuse_next_ln(g, ln(LN2, l, i, nullptr));
        return g;
      });
      const bool fused = r.mlp2(p0.p, p2.p, M, "proj");  // (nothing launched when it returns false)
      ln2_done = fused && ln2_fuse;
      if (!fused) {
        r.fgemm(p0, EPI_BIAS_TANH_BF16, "proj0");
        for (int i = 0; i < M; ++i) p2.p[i].lnf_y = nullptr;  // the plain GEMM runs no LayerNorm
        r.fgemm(p2, EPI_BIAS_RESID_F32, "proj2");
      }
    }
    if (!ln2_done)
      r.ok(mmt_launch_ln_fwd(lns(M, [&](int i) { return ln(LN2, l, i, r.f32(a[i].x1)); }), R, C, r.s), "ln2_fwd");
    // FFN (model.py:162-175, 225)
    GemmBatch f0 = gemms(M, [&](int i) {
      Lin g = lin(a[i].c, a[i].c8, a[i].cs8, C, ldsC, x[i].F0, x[i].bf0).out16(r.b16(a[i].f), 4 * C);
      if (c->relu_bits) { g.mask8 = r.W<uint8_t>(a[i].fm); g.ldm8 = 4 * C / 8; }
      if (f8) { g.o8 = r.W<uint8_t>(a[i].f8); g.ld8 = 4 * C; g.s8 = r.W<uint8_t>(a[i].fs8); g.lds8 = ldsF; }
      return g;
    });
    GemmBatch f2 = gemms(M, [&](int i) {
      Lin g = lin(a[i].f, a[i].f8, a[i].fs8, 4 * C, ldsF, x[i].F2, x[i].bf2).out32(r.f32(a[i].x2), C, r.f32(a[i].x1));
      if (c->any_cross) g.out16(r.b16(a[i].x2h), C);
      r.set_drop(g, l, i, DS_FFN);
      // the LayerNorm that reads this problem's x2 next: lnc (cross-attention query side), else the
      // next layer's ln1, else (last layer) the post block's
      if (fuse_fwd) {
        const PostRows w = post_rows(i);
        fuse_next_ln(g, x[i].cross ? ln(LNC, l, i, nullptr) : l + 1 < c->L ? ln(LN1, l + 1, i, nullptr)
                        : ln_fwd_problem(nullptr, r.P(c->post[i].lnw), r.P(c->post[i].lnb), w.y, w.mean, w.rstd));
      }
      return g;
    });
    // both products as one launch (mmt_set_ffn_fused; C = 256, bf16, no ReLU bits: ffn_fwd_kernel, the bits of
    // the pair below); false (nothing launched) for every other shape or a field it does not implement
    const bool ffn_one = !f8 && !c->relu_bits && C == 256 && kn.ffn_fused != 0 && r.ffn(f0.p, f2.p, M, "ffn");
    if (!ffn_one) r.fgemm(f0, EPI_BIAS_RELU_BF16, "ffn0", f8);
    bool lnc_done = false;
    if (fuse_fwd && (ffn_one || r.gemm_resid_ln(f2, "ffn2"))) {
      for (int i = 0; i < M; ++i) {
        if (x[i].cross) lnc_done = true;
        else if (l + 1 < c->L) ln1_done[i] = 1;
        else lnf_done[i] = 1;
      }
    } else if (!ffn_one) {
      for (int i = 0; i < M; ++i) f2.p[i].lnf_y = nullptr;  // the plain GEMM runs no LayerNorm
      r.fgemm(f2, EPI_BIAS_RESID_F32, "ffn2", f8);
    }
    std::vector<const float*> xout(M);
    for (int i = 0; i < M; ++i) xout[i] = r.f32(a[i].x2);
    if (c->any_cross) {
      const std::vector<int> cx = cross_set(x, M);
      const int nc = (int)cx.size();
      if (!lnc_done)
        r.ok(mmt_launch_ln_fwd(lns(nc, [&](int u) { return ln(LNC, l, cx[u], r.f32(a[cx[u]].x2)); }), R, C, r.s),
             "lnc_fwd");
      r.fgemm(gemms(nc, [&](int u) {
                const int i = cx[u];
                return lin(a[i].d, a[i].d8, a[i].ds8, C, ldsC, x[i].Wq, -1).out16(r.b16(a[i].qc), C);
              }), EPI_STORE_BF16, "ca_q", f8);
      // KV projections of the other modalities' post-FFN states, grouped up to 8 per launch
      GemmBatch gk{};
      for_each_cross_kv(cx, M, false,
                        [&](int i, int j, int jj) {
                          gk.p[gk.count++] = r.linear(r.b16(a[j].x2h), C, x[i].Wkv[jj], -1).out16(r.b16(a[i].kv[jj]), 2 * C);
                        },
                        [&] { r.fgemm(gk, EPI_STORE_BF16, "ca_kv"); gk = GemmBatch{}; });
      r.attn(batch_of<AttnBatch>(nc, [&](int u) { return r.cross_attn(a[cx[u]], l, cx[u]); }), false, scale, "ca_attn_fwd");
      GemmBatch c0 = gemms(nc, [&](int u) {
        const int i = cx[u];
        return r.linear(r.b16(a[i].oc), C, x[i].C0, x[i].bc0).out16(r.b16(a[i].pc), ldp);
      });
      GemmBatch c2 = gemms(nc, [&](int u) {
        const int i = cx[u];
        Lin g = r.linear(r.b16(a[i].pc), ldp, x[i].C2, x[i].bc2).out32(r.f32(a[i].x3), C, r.f32(a[i].x2));
        r.set_drop(g, l, i, DS_CA_PROJ);
        return g;
      });
      for (int i : cx) xout[i] = r.f32(a[i].x3);
      if (!r.mlp2(c0.p, c2.p, nc, "ca_proj")) {
        r.fgemm(c0, EPI_BIAS_TANH_BF16, "ca_proj0");
        r.fgemm(c2, EPI_BIAS_RESID_F32, "ca_proj2");
      }
    }
    xin = xout;
  }
  if (r.rc != MMT_OK) return r.rc;
  // post block + CE
  LnBatch lf{};
  if (tgt) {  // the loss accumulators and this forward's flag word, zeroed by the LN launch
    lf.zero_f = losses; lf.nzero_f = M;
    lf.zero_i = r.W<int>(p.flag); lf.nzero_i = 1;
  }
  static const char* const post_labels[3] = {"lnf_fwd", "head0", "head2"};
  run_post(c, r, R, xin, lnf_done.data(), post_rows, logits, lf, post_labels);
  if (tgt && r.rc == MMT_OK && c->loss_on) {
    // the objective of mmt_set_loss: D of the weighted modalities (doubles behind the two flag words of the flag
    // block), then the loss kernel that writes dlogits times R / D: the backward is the plain loss's
    CeSpecBatch sb{}; sb.count = M;
    double* denom = reinterpret_cast<double*>(r.W<char>(p.flag) + LOSS_DENOM_OFF);
    for (int i = 0; i < M; ++i) {
      CeProblem& q = sb.p[i].ce;
      q.logits = logits[i]; q.tgt = tgt[i]; q.dlogits = r.b16(p.dlog[i]);
      q.loss = losses + i; q.V = c->V[i]; q.ld_d = c->ldv[i];
      q.flag = r.W<int>(p.flag); q.bit = 1 << i;
      q.part = r.f32(p.celoss[i]);
      const mmt_loss_spec& ls = c->loss[i];
      sb.p[i].eps = ls.label_smoothing; sb.p[i].cw = ls.class_weight; sb.p[i].pw = ls.position_weight;
      sb.p[i].denom = (ls.class_weight || ls.position_weight) ? denom + i : nullptr;
    }
    bool weights = false;
    for (int i = 0; i < M; ++i) weights = weights || sb.p[i].denom;
    auto no_cost = [](double*, double*) {};
    if (weights) r.launch("ce_denom", r.s, [&] { return mmt_launch_ce_denom(sb, R, c->T, r.s); }, no_cost);
    r.launch("ce_fwd", r.s, [&] { return mmt_launch_ce_spec(sb, R, c->T, r.s); }, no_cost);
  } else if (tgt && r.rc == MMT_OK) {
    CeBatch cb{}; cb.count = M;
    for (int i = 0; i < M; ++i) {
      cb.p[i].logits = logits[i]; cb.p[i].tgt = tgt[i]; cb.p[i].dlogits = r.b16(p.dlog[i]);
      cb.p[i].loss = losses + i; cb.p[i].V = c->V[i]; cb.p[i].ld_d = c->ldv[i];
      cb.p[i].flag = r.W<int>(p.flag); cb.p[i].bit = 1 << i;
      cb.p[i].part = r.f32(p.celoss[i]);
    }
    r.launch("ce_fwd", r.s, [&] { return mmt_launch_ce_fwd(cb, R, r.s); }, [](double*, double*) {});
  }
  return r.rc;
}

// -------------------------------------------------------------------------------------------
// KV-cache decode (generate, reference model.py:404-446): the forward of ONE new position t per
// sequence, every layer and modality, on compact [B, *] rows. The self- and cross-attention keys /
// values of positions < t are the ones the prefill forward (mmt_forward, same workspace) left in
// its saved Q/K/V and cross-K/V buffers (row b*T + s); this step appends row t to them and runs
// the decode attention over 0..t. Eval semantics (no dropout). The packed bf16 weights are the
// ones the prefill forward made.
//
// Where the compact rows live is the caller's (DecWhere): the workspace plan with B rows (mmt_decode_step), or a
// fan buffer with B*S rows, row b*S + s being sample s of prompt b (mmt_decode_fanout_step). The fan-out step
// leaves the workspace alone: keys / values of positions < n0 are read from the cache rows of sequence b,
// position t is appended to the fan buffer's tails (row r*max_new + t - n0) and the attention is the fan-out
// kernel. Everything else is the same launches over `rows` rows.
//
// The rolling step (mmt_rolling_step, roll_m > 0) is the same walk over B*S*m rows, row r*m + i being tail position
// i of path r = b*S + s at sequence position roll_p + i: the embedding reads token i of row r of the caller's
// [B*S, idx_ld] buffers, stage 2 and the cross-K/V projections write all m positions of every path, which makes the
// compact K|Q|V and cross-K/V rows of the layer in flight the paths' tails (row r*m + i), and the attention is the
// rolling fan-out kernel over the roll_p cache rows and those tails. The residual rows of layer l live in slot
// l % xlayers; the post block runs over the B*S last tail rows, gathered to `last`. Its launches carry roll_* labels.
// -------------------------------------------------------------------------------------------
struct DecWhere {
  char* base; const Plan::Dec* dec; const size_t* dec_x; int rows;
  const FanPlan* fan = nullptr; int S = 1, n0 = 0;
  int xlayers = 0;  // layer slots of dec_x (0: one per layer)
  int roll_p = 0, roll_m = 0; int64_t idx_ld = 0; const size_t* last = nullptr;
  template <class T>
  T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};

int run_decode(mmt_ctx* c, Runner& r, const DecWhere& w, int t, const int64_t* const* idx, float* const* logits) {
  const int M = c->M, C = c->C, H = c->H, hs = c->hs, B = r.B, T = c->T;
  const int R = w.rows;  // compact rows (== r.R)
  const int ldh1 = r8(3 * H * c->hh), ldp = r8(C / 2);
  const float scale = 1.0f / std::sqrt((float)hs);
  Plan& p = c->plan;
  r.wpk = r.b16(p.pack);
  auto D = [&](size_t off) { return w.at<bf16_t>(off); };  // compact bf16 rows
  auto scatter_rows = [&](bf16_t* cache, int ld, const bf16_t* rows, const char* what) {
    // compact row b -> cache row b*T + t
    r.ok(hipMemcpy2DAsync(cache + (size_t)t * ld, (size_t)T * ld * 2, rows, (size_t)ld * 2, (size_t)ld * 2, B,
                          hipMemcpyDeviceToDevice, r.s), what);
  };
  const int tail_rows = w.fan ? w.fan->max_new : 0;
  const int rm = w.roll_m;  // > 0: the rolling step
  auto lb = [&](const char* dec, const char* roll) { return rm ? roll : dec; };
  auto tail_append = [&](bf16_t* tail, int ld, const bf16_t* rows, const char* what) {
    // compact row r -> tail row r*max_new + (t - n0)
    r.ok(hipMemcpy2DAsync(tail + (size_t)(t - w.n0) * ld, (size_t)tail_rows * ld * 2, rows, (size_t)ld * 2,
                          (size_t)ld * 2, R, hipMemcpyDeviceToDevice, r.s), what);
  };
  // every LayerNorm of the step writes the same compact rows: y as given, the statistics (unused) in d.mean / d.rstd
  auto ln = [&](int i, const float* xi, int64_t gamma, int64_t beta, size_t y) {
    return ln_fwd_problem(xi, r.P(gamma), r.P(beta), D(y), w.at<float>(w.dec[i].mean), w.at<float>(w.dec[i].rstd));
  };
  {
    EmbBatch eb{};
    eb.count = M;
    for (int i = 0; i < M; ++i) {
      eb.p[i].idx = idx[i]; eb.p[i].tok = r.P(c->post[i].tok); eb.p[i].pos = r.P(c->pos_off) + (int64_t)t * C;
      eb.p[i].x = w.at<float>(w.dec[i].x0); eb.p[i].V = c->V[i];
      eb.p[i].idx_ld = w.idx_ld;  // rolling: token i of path r at idx[i][r * idx_ld + i], position t + i
    }
    r.ok(rm ? mmt_launch_embed_fwd(eb, R / rm, rm, C, r.s) : mmt_launch_embed_fwd(eb, R, 1, C, r.s),
         lb("dec_embed", "roll_embed"));
  }
  std::vector<const float*> xin(M);
  for (int i = 0; i < M; ++i) xin[i] = w.at<float>(w.dec[i].x0);
  for (int l = 0; l < c->L && r.rc == MMT_OK; ++l) {
    const LM* x = &c->lm[(size_t)l * M];
    const ActLM* a = &p.act[(size_t)l * M];
    const Plan::Dec* d = w.dec;
    const size_t lx = w.xlayers ? l % w.xlayers : l;
    auto X = [&](int i, int k) { return w.at<float>(w.dec_x[(lx * M + i) * 3 + k]); };
    r.ok(mmt_launch_ln_fwd(lns(M, [&](int i) { return ln(i, xin[i], x[i].ln1w, x[i].ln1b, d[i].a16); }), R, C, r.s),
         lb("dec_ln1", "roll_ln1"));
    r.fgemm(gemms(M, [&](int i) { return r.linear(D(d[i].a16), C, x[i].W1, x[i].b1).out16(D(d[i].h1), ldh1); }),
            EPI_BIAS_TANH_BF16, lb("dec_qkv1", "roll_qkv1"));
    Qkv2Batch qb{}; qb.count = M;
    for (int i = 0; i < M; ++i) {
      qb.p[i].h1 = D(d[i].h1); qb.p[i].w2 = r.P(x[i].w2); qb.p[i].out = D(d[i].qkv);
      // fan-out: stage 2 writes row t - n0 of the self-attention tail itself (leading dimension max_new * 3C; the
      // kernel forms (int64) row * ld and writes the 3C columns only), so no append copy and no compact K|Q|V row
      if (w.fan) qb.p[i].out = D(w.fan->sa_tail[(size_t)l * M + i]) + (size_t)(t - w.n0) * 3 * C;
    }
    r.ok(mmt_launch_qkv2_fwd(qb, R, 3 * H, hs, ldh1, w.fan ? tail_rows * 3 * C : 3 * C, r.s),
         lb("dec_qkv2", "roll_qkv2"));
    if (rm) {
      const FanoutAttnBatch fb = batch_of<FanoutAttnBatch>(M, [&](int i) {
        FanoutAttnProblem q{};
        bf16_t* tail = D(d[i].qkv);  // the K|Q|V rows stage 2 just wrote: queries and tails at once
        self_attn_io(q, tail + C, 3 * C, r.b16(a[i].qkv), D(d[i].o16), C, hs);
        q.tk[0] = tail; q.tv[0] = tail + 2 * C; q.tail_ld = 3 * C;
        return q;
      });
      r.ok(mmt_launch_attn_rolling_fanout(fb, B, w.S, w.roll_p, rm, T, H, hs, scale, r.s), "roll_attn");
    } else if (w.fan) {
      const FanoutAttnBatch fb = batch_of<FanoutAttnBatch>(M, [&](int i) {
        FanoutAttnProblem q{};
        bf16_t* tail = D(w.fan->sa_tail[(size_t)l * M + i]);
        // the query: the tail row just written
        self_attn_io(q, tail + (size_t)(t - w.n0) * 3 * C + C, tail_rows * 3 * C, r.b16(a[i].qkv), D(d[i].o16), C, hs);
        q.tk[0] = tail; q.tv[0] = tail + 2 * C; q.tail_ld = 3 * C;
        return q;
      });
      r.ok(mmt_launch_attn_decode_fanout(fb, B, w.S, w.n0, t, T, H, hs, tail_rows, scale, r.s), "fan_attn");
    } else {
      const DecodeAttnBatch ab = batch_of<DecodeAttnBatch>(M, [&](int i) {
        DecodeAttnProblem q{};
        scatter_rows(r.b16(a[i].qkv), 3 * C, D(d[i].qkv), "dec_kv_append");
        self_attn_io(q, D(d[i].qkv) + C, 3 * C, r.b16(a[i].qkv), D(d[i].o16), C, hs);
        return q;
      });
      r.ok(mmt_launch_attn_decode(ab, B, t, T, H, hs, scale, r.s), "dec_attn");
    }
    r.fgemm(gemms(M, [&](int i) { return r.linear(D(d[i].o16), C, x[i].P0, x[i].bp0).out16(D(d[i].p1), ldp); }),
            EPI_BIAS_TANH_BF16, lb("dec_proj0", "roll_proj0"));
    r.fgemm(gemms(M, [&](int i) { return r.linear(D(d[i].p1), ldp, x[i].P2, x[i].bp2).out32(X(i, 0), C, xin[i]); }),
            EPI_BIAS_RESID_F32, lb("dec_proj2", "roll_proj2"));
    r.ok(mmt_launch_ln_fwd(lns(M, [&](int i) { return ln(i, X(i, 0), x[i].ln2w, x[i].ln2b, d[i].a16); }), R, C, r.s),
         lb("dec_ln2", "roll_ln2"));
    r.fgemm(gemms(M, [&](int i) { return r.linear(D(d[i].a16), C, x[i].F0, x[i].bf0).out16(D(d[i].f), 4 * C); }),
            EPI_BIAS_RELU_BF16, lb("dec_ffn0", "roll_ffn0"));
    r.fgemm(gemms(M, [&](int i) {
              Lin g = r.linear(D(d[i].f), 4 * C, x[i].F2, x[i].bf2).out32(X(i, 1), C, X(i, 0));
              if (c->any_cross) g.out16(D(d[i].x2h), C);
              return g;
            }), EPI_BIAS_RESID_F32, lb("dec_ffn2", "roll_ffn2"));
    std::vector<const float*> xout(M);
    for (int i = 0; i < M; ++i) xout[i] = X(i, 1);
    if (c->any_cross) {
      const std::vector<int> cx = cross_set(x, M);
      const int nc = (int)cx.size();
      r.ok(mmt_launch_ln_fwd(lns(nc, [&](int u) {
                               const int i = cx[u];
                               return ln(i, X(i, 1), x[i].lncw, x[i].lncb, d[i].d16);
                             }), R, C, r.s), lb("dec_lnc", "roll_lnc"));
      r.fgemm(gemms(nc, [&](int u) {
                const int i = cx[u];
                return r.linear(D(d[i].d16), C, x[i].Wq, -1).out16(D(d[i].qc), C);
              }), EPI_STORE_BF16, lb("dec_ca_q", "roll_ca_q"));
      GemmBatch gk{};
      for_each_cross_kv(cx, M, false,
                        [&](int i, int j, int jj) {
                          gk.p[gk.count++] = r.linear(D(d[j].x2h), C, x[i].Wkv[jj], -1).out16(D(d[i].kv[jj]), 2 * C);
                        },
                        [&] { r.fgemm(gk, EPI_STORE_BF16, lb("dec_ca_kv", "roll_ca_kv")); gk = GemmBatch{}; });
      if (rm) {
        const FanoutAttnBatch fb = batch_of<FanoutAttnBatch>(nc, [&](int u) {
          const int i = cx[u];
          FanoutAttnProblem q{};
          cross_attn_io(q, D(d[i].qc), [&](int j) { return r.b16(a[i].kv[j]); }, M - 1, D(d[i].oc), C, hs);
          for (int j = 0; j < M - 1; ++j) { q.tk[j] = D(d[i].kv[j]); q.tv[j] = q.tk[j] + hs; }  // the rows just made
          q.tail_ld = 2 * C;
          return q;
        });
        r.ok(mmt_launch_attn_rolling_fanout(fb, B, w.S, w.roll_p, rm, T, H, hs, scale, r.s), "roll_ca_attn");
      } else if (w.fan) {
        const FanoutAttnBatch fb = batch_of<FanoutAttnBatch>(nc, [&](int u) {
          const int i = cx[u];
          FanoutAttnProblem q{};
          cross_attn_io(q, D(d[i].qc), [&](int j) { return r.b16(a[i].kv[j]); }, M - 1, D(d[i].oc), C, hs);
          for (int j = 0; j < M - 1; ++j) {
            bf16_t* tail = D(w.fan->ca_tail[((size_t)l * M + i) * MAXM + j]);
            tail_append(tail, 2 * C, D(d[i].kv[j]), "fan_cakv_append");
            q.tk[j] = tail; q.tv[j] = tail + hs;
          }
          q.tail_ld = 2 * C;
          return q;
        });
        r.ok(mmt_launch_attn_decode_fanout(fb, B, w.S, w.n0, t, T, H, hs, tail_rows, scale, r.s), "fan_ca_attn");
      } else {
        const DecodeAttnBatch cb = batch_of<DecodeAttnBatch>(nc, [&](int u) {
          const int i = cx[u];
          DecodeAttnProblem q{};
          for (int j = 0; j < M - 1; ++j) scatter_rows(r.b16(a[i].kv[j]), 2 * C, D(d[i].kv[j]), "dec_cakv_append");
          cross_attn_io(q, D(d[i].qc), [&](int j) { return r.b16(a[i].kv[j]); }, M - 1, D(d[i].oc), C, hs);
          return q;
        });
        r.ok(mmt_launch_attn_decode(cb, B, t, T, H, hs, scale, r.s), "dec_ca_attn");
      }
      r.fgemm(gemms(nc, [&](int u) {
                const int i = cx[u];
                return r.linear(D(d[i].oc), C, x[i].C0, x[i].bc0).out16(D(d[i].pc), ldp);
              }), EPI_BIAS_TANH_BF16, lb("dec_ca_proj0", "roll_ca_proj0"));
      r.fgemm(gemms(nc, [&](int u) {
                const int i = cx[u];
                return r.linear(D(d[i].pc), ldp, x[i].C2, x[i].bc2).out32(X(i, 2), C, X(i, 1));
              }), EPI_BIAS_RESID_F32, lb("dec_ca_proj2", "roll_ca_proj2"));
      for (int i : cx) xout[i] = X(i, 2);
    }
    xin = xout;
  }
  if (r.rc != MMT_OK) return r.rc;
  if (rm) {
    // the post block over the paths' last tail rows only: fp32 row r*m + m - 1 -> row r of `last`
    const int paths = R / rm;
    for (int i = 0; i < M; ++i) {
      float* dst = w.at<float>(w.last[i]);
      r.ok(hipMemcpy2DAsync(dst, (size_t)C * 4, xin[i] + (size_t)(rm - 1) * C, (size_t)rm * C * 4, (size_t)C * 4, paths,
                            hipMemcpyDeviceToDevice, r.s), "roll_last_rows");
      xin[i] = dst;
    }
    if (r.rc != MMT_OK) return r.rc;
    r.R = paths;
    static const char* const roll_labels[3] = {"roll_lnf", "roll_head0", "roll_head2"};
    run_post(c, r, paths, xin, nullptr,
             [&](int i) {
               const Plan::Dec& d = w.dec[i];
               return PostRows{D(d.lnf16), w.at<float>(d.mean), w.at<float>(d.rstd), D(d.hh)};
             },
             logits, LnBatch{}, roll_labels);
    return r.rc;
  }
  static const char* const post_labels[3] = {"dec_lnf", "dec_head0", "dec_head2"};
  run_post(c, r, R, xin, nullptr,
           [&](int i) {
             const Plan::Dec& d = w.dec[i];
             return PostRows{D(d.lnf16), w.at<float>(d.mean), w.at<float>(d.rstd), D(d.hh)};
           },
           logits, LnBatch{}, post_labels);
  return r.rc;
}

// -------------------------------------------------------------------------------------------
// backward stages: 0 = post block, 1..L = layers L-1..0, L+1 = embeddings
// -------------------------------------------------------------------------------------------
void colsum_add(Runner& r, ColsumBatch& cb, int u, const bf16_t* x, int ld, float* out, int N, const float* aptr,
                float alpha) {
  cb.p[u].x = x; cb.p[u].ld = ld; cb.p[u].out = out; cb.p[u].N = N; cb.p[u].alpha_ptr = aptr; cb.p[u].alpha = alpha;
}

// The bf16 residual-gradient copy dres16 written by a LayerNorm backward feeds the dropped
// branch that precedes it (layer lprev): its CA projection (cross modalities of a model with
// cross-attention), else its FFN. The copy carries that branch's dropout mask and its column
// sums are that branch's output-bias gradient. Modalities whose copy is rebuilt later (non-cross
// modalities of a cross model) and lprev < 0 (embeddings) get no copy.
// current dres16 copy (the last one written), and the next one in the rotation (for a writer)
inline bf16_t* d16_cur(mmt_ctx* c, Runner& r, int i) { return r.W<bf16_t>(c->plan.dres16[c->d16 & 7][i]); }
inline void d16_advance(mmt_ctx* c) { ++c->d16; }

void set_dres16_consumer(mmt_ctx* c, Runner& r, LnProblem& lp, int i, int lprev, float* grads) {
  lp.dx16 = nullptr; lp.dsum = nullptr;
  lp.drop_key = 0; lp.drop_thr = 0; lp.drop_scale = 1.f;
  if (lprev < 0) return;
  const LM& x = c->lm[(size_t)lprev * c->M + i];
  if (c->any_cross) {
    if (!x.cross) return;
    r.set_drop(lp, lprev, i, DS_CA_PROJ);
    lp.dsum = grads + x.bc2;
  } else {
    r.set_drop(lp, lprev, i, DS_FFN);
    lp.dsum = grads + x.bf2;
  }
  lp.dx16 = d16_cur(c, r, i);  // the caller advanced the rotation for this launch
}

int run_backward_stage(mmt_ctx* c, Runner& r, int stage, const float* loss_grads, float* grads) {
  const int M = c->M, C = c->C, H = c->H, hs = c->hs, R = r.R, T = c->T, L = c->L;
  const int ldh1 = r8(3 * H * c->hh), ldp = r8(C / 2);
  const float scale = 1.0f / std::sqrt((float)hs);
  const Knobs& kn = knobs();
  Plan& p = c->plan;
  const bf16_t* wpk = r.b16(p.pack);
  const int par = stage & 1;  // copy of the side-stream-read scratch this stage writes (Plan)
  // one Linear's two gradients from the rows g = dY (ld ldy): dW += dY^T X, and dX = dY W (the caller adds where it goes)
  auto dw_of = [&](const bf16_t* g, int ldy, size_t x16, int ldx, const Mat& W) {
    return gp_dw(g, ldy, r.b16(x16), ldx, grads, W, R);
  };
  auto dx_of = [&](const bf16_t* g, int ldy, const Mat& W) { return gp_dx(g, ldy, wpk, W, R); };
  // ... dX as fp32 rows in dln (the input of the LayerNorm backward that follows), or as bf16 rows through the
  // activation's derivative (aux: the saved activation) with the previous Linear's bias gradient as column sums
  auto dx_ln = [&](const bf16_t* g, int ldy, const Mat& W, int i) {
    GemmProblem d = dx_of(g, ldy, W);
    d.o32 = r.f32(p.dln[i]); d.ldc = C;
    return d;
  };
  auto dx_act = [&](const bf16_t* g, int ldy, const Mat& W, size_t aux, size_t out, int ld, int64_t dbias) {
    GemmProblem d = dx_of(g, ldy, W);
    d.aux = r.b16(aux); d.ldaux = ld; d.o16 = r.b16(out); d.ldo16 = ld; d.dbias = grads + dbias;
    return d;
  };
  auto dx_16 = [&](const bf16_t* g, int ldy, const Mat& W, size_t out, int ld) {
    GemmProblem d = dx_of(g, ldy, W);
    d.o16 = r.b16(out); d.ldo16 = ld;
    return d;
  };
  if (stage == 0) {
    c->d16 = 0;
    // the active prefix only; in-place accumulation (mmt_set_grad_accumulate) adds to what is there
    if (!c->grad_accum) HIPCHK(c, hipMemsetAsync(grads, 0, sizeof(float) * c->nactive, r.s));
    // the token-table gradient's row sort (stable: a fixed summation order) needs only the forward's
    // token ids: it runs now on the side stream, off the critical path (27.6 us serial at C1 as the
    // embedding stage's first launch in round 5)
    c->emb_sorted = false;
    {
      EmbBatch eb{}; eb.count = M;
      for (int i = 0; i < M; ++i) {
        eb.p[i].idx = c->last_idx[i]; eb.p[i].V = c->V[i]; eb.p[i].perm = r.W<int>(p.eperm[i]);
      }
      if (mmt_emb_sort_ok(eb, R, C)) {
        if (!c->emb_ev) HIPCHK(c, hipEventCreateWithFlags(&c->emb_ev, hipEventDisableTiming));
        const hipStream_t ss = r.side_stream() ? r.side() : r.s;
        if (r.ok(mmt_launch_emb_sort(eb, R, ss), "emb_sort") && r.ok(hipEventRecord(c->emb_ev, ss), "event record"))
          c->emb_sorted = true;
      }
    }
    const float invR = 1.0f / (float)R;
    auto scaled = [&](GemmProblem g, int i) { g.alpha_ptr = loss_grads + i; g.alpha = invR; return g; };
    r.dwgemm(gemms(M, [&](int i) {
               return scaled(dw_of(r.b16(p.dlog[i]), c->ldv[i], p.hh[i], c->ldvh[i], c->post[i].H2), i);
             }), "head2_dw");
    ColsumBatch cs{}; cs.count = M;
    for (int i = 0; i < M; ++i)
      colsum_add(r, cs, i, r.b16(p.dlog[i]), c->ldv[i], grads + c->post[i].b2, c->V[i], loss_grads + i, invR);
    r.det_arm(cs);
    r.ok(mmt_launch_colsum(cs, R, r.s), "head2_db");
    r.gemm(gemms(M, [&](int i) {  // (head0 bias grad fused)
             const PostM& q = c->post[i];
             return scaled(dx_act(r.b16(p.dlog[i]), c->ldv[i], q.H2, p.hh[i], p.gbig[par][i], c->ldvh[i], q.b0), i);
           }), true, false, EPI_DTANH_BF16, 1, "head2_dx");
    r.dwgemm(gemms(M, [&](int i) { return dw_of(r.b16(p.gbig[par][i]), c->ldvh[i], p.lnf16[i], C, c->post[i].H0); }),
             "head0_dw");
    r.flush();
    d16_advance(c);
    const LnBatch lb = lns(M, [&](int i) {
      const ActLM& a = p.act[(size_t)(L - 1) * M + i];
      const float* xfin = (L == 0) ? r.f32(p.xemb[i]) : (c->lm[(size_t)(L - 1) * M + i].cross ? r.f32(a.x3) : r.f32(a.x2));
      r.ok(hipMemsetAsync(r.f32(p.dres[i]), 0, sizeof(float) * (size_t)R * C, r.s), "memset dres");
      LnProblem q = ln_bwd_problem(xfin, r.P(c->post[i].lnw), r.f32(p.meanf[i]), r.f32(p.rstdf[i]), r.f32(p.dln[i]),
                                   r.f32(p.dres[i]), grads + c->post[i].lnw, grads + c->post[i].lnb);
      set_dres16_consumer(c, r, q, i, L - 1, grads);
      return q;
    });
    r.gemm_ln_bwd(gemms(M, [&](int i) { return dx_ln(r.b16(p.gbig[par][i]), c->ldvh[i], c->post[i].H0, i); }), lb,
                  R, C, "head0_dx", "lnf_bwd");
    return r.rc;
  }
  // layer stage
  const int l = L - stage;
  const LM* x = &c->lm[(size_t)l * M];
  const ActLM* a = &p.act[(size_t)l * M];
  std::vector<const float*> xin(M);
  for (int i = 0; i < M; ++i) {
    if (l == 0) xin[i] = r.f32(p.xemb[i]);
    else {
      const ActLM& pa = p.act[(size_t)(l - 1) * M + i];
      xin[i] = c->lm[(size_t)(l - 1) * M + i].cross ? r.f32(pa.x3) : r.f32(pa.x2);
    }
  }
  // the backward of this layer's LayerNorm n on modality i (input rows xi): dy in dln, dx added to dres
  auto ln_bwd = [&](const LnSite& n, int i, const float* xi) {
    return ln_bwd_problem(xi, r.P(x[i].*n.w), r.f32(a[i].*n.mean), r.f32(a[i].*n.rstd), r.f32(p.dln[i]), r.f32(p.dres[i]),
                          grads + x[i].*n.w, grads + x[i].*n.b);
  };
  // the backward of an out-projection pair (self- or cross-attention's: weights P0 / P2 or C0 / C2) of the n
  // modalities at_(u), hidden rows a.*hid and input rows a.*in: the dres16 copy carries the projection's dropout mask (its output-bias grad came with it);
  // both data gradients in one launch where the fused kernel takes the shape (C = 256 / 512), else two GEMMs
  auto proj_bwd = [&](int n, auto&& at_, auto&& mats, size_t ActLM::*hid, size_t ActLM::*in, size_t (*gp)[MAXM],
                      const char* const (&lab)[5]) {
    GemmBatch dx2 = gemms(n, [&](int u) {
      const int i = at_(u);
      return dx_act(d16_cur(c, r, i), C, *mats(i).w2, a[i].*hid, gp[par][i], ldp, mats(i).b0);
    });
    r.dwgemm(gemms(n, [&](int u) { const int i = at_(u); return dw_of(d16_cur(c, r, i), C, a[i].*hid, ldp, *mats(i).w2); }),
             lab[0]);
    GemmBatch dx0 = gemms(n, [&](int u) { const int i = at_(u); return dx_16(r.b16(gp[par][i]), ldp, *mats(i).w0, p.gdo[i], C); });
    const bool fused = r.mlp2(dx2.p, dx0.p, n, lab[1], true);
    if (!fused) r.gemm(dx2, true, false, EPI_DTANH_BF16, 1, lab[2]);
    r.dwgemm(gemms(n, [&](int u) { const int i = at_(u); return dw_of(r.b16(gp[par][i]), ldp, a[i].*in, C, *mats(i).w0); }),
             lab[3]);
    if (!fused) r.gemm(dx0, true, false, EPI_STORE_BF16, 1, lab[4]);
    r.flush();
  };
  struct ProjMats { const Mat* w0; const Mat* w2; int64_t b0; };
  if (c->any_cross) {
    const std::vector<int> cx = cross_set(x, M);
    const int nc = (int)cx.size();
    static const char* const ca_labels[5] = {"ca_proj2_dw", "ca_proj_dx", "ca_proj2_dx", "ca_proj0_dw", "ca_proj0_dx"};
    proj_bwd(nc, [&](int u) { return cx[u]; }, [&](int i) { return ProjMats{&x[i].C0, &x[i].C2, x[i].bc0}; }, &ActLM::pc,
             &ActLM::oc, p.gpc, ca_labels);
    r.attn(batch_of<AttnBatch>(nc, [&](int u) {
             const int i = cx[u];
             AttnProblem q = r.cross_attn(a[i], l, i);
             for (int j = 0; j < M - 1; ++j) {
               q.dvec[j] = r.f32(p.dvec[i][j]);
               bf16_t* dkv = r.b16(p.dkv[par][i][j]);
               q.dk[j] = dkv; q.dv[j] = dkv + hs;
             }
             q.dout = r.b16(p.gdo[i]); q.dout_ld = C; q.dq = r.b16(p.gq[par][i]); q.dq_ld = C;
             // fp32 rows for the one-pass hs-32 backward's dQ sum over the KV streams: dln is free here (the
             // cross-query dX GEMM after the attention writes it)
             q.dq32 = r.f32(p.dln[i]); q.dq32_ld = C;
             q.dkv_ld = 2 * C; q.dkv_hstride = 2 * hs;
             return q;
           }), true, scale, "ca_attn_bwd");
    r.dwgemm(gemms(nc, [&](int u) { const int i = cx[u]; return dw_of(r.b16(p.gq[par][i]), C, a[i].d, C, x[i].Wq); }),
             "ca_q_dw");
    r.gemm_ln_bwd(gemms(nc, [&](int u) { const int i = cx[u]; return dx_ln(r.b16(p.gq[par][i]), C, x[i].Wq, i); }),
                  lns(nc, [&](int u) { return ln_bwd(LNC, cx[u], r.f32(a[cx[u]].x2)); }), R, C, "ca_q_dx", "lnc_bwd");
    // KV projections: dWkv += dkv^T x2_j ; dres[j] += dkv Wkv (one launch per query modality:
    // different query modalities accumulate into the same dres[j]). The LAST query modality that
    // accumulates into dres[j] also writes its bf16 copy for the FFN backward in that epilogue (FFN
    // dropout mask, FFN output-bias gradient as column sums): a separate drop_copy pass re-read the
    // fp32 rows (6 x 38 us per step at the target). Only a modality no launch accumulates into (one
    // cross modality: its own dres) keeps the copy pass (Knobs: MMT_DROP_COPY_FUSE = 0: every modality does).
    const bool fuse_copy = kn.drop_copy_fuse != 0;
    d16_advance(c);
    std::vector<int> last_writer(M, -1);
    for (int i : cx)
      for (int j = 0; j < M; ++j)
        if (j != i) last_writer[j] = i;
    // the fused copy is only right if no later launch of this stage accumulates into dres[j] (the FFN
    // backward reads the copy): launches run in cx order and last_writer[j] is the last i of cx that
    // writes dres[j]; copied[j] checks that invariant as the launches are built
    std::vector<char> copied(M, 0);
    GemmBatch kw{}, kx{};
    for_each_cross_kv(cx, M, true,
                      [&](int i, int j, int jj) {
                        if (copied[j] && r.rc == MMT_OK)
                          r.rc = fail(c, MMT_ERR_STATE, "cross K/V dX: dres written after its fused bf16 copy");
                        const bf16_t* g = r.b16(p.dkv[par][i][jj]);
                        kw.p[kw.count++] = dw_of(g, 2 * C, a[j].x2h, C, x[i].Wkv[jj]);
                        GemmProblem d = dx_of(g, 2 * C, x[i].Wkv[jj]);
                        d.o32 = r.f32(p.dres[j]); d.ldc = C;
                        if (last_writer[j] == i && fuse_copy) {
                          copied[j] = 1;
                          d.o16 = d16_cur(c, r, j); d.ldo16 = C; d.dbias = grads + x[j].bf2;
                          r.set_drop(d, l, j, DS_FFN);
                        }
                        kx.p[kx.count++] = d;
                      },
                      [&] {
                        r.dwgemm(kw, "ca_kv_dw");
                        r.gemm(kx, true, false, EPI_ACC_F32, 1, "ca_kv_dx");
                        kw = GemmBatch{}; kx = GemmBatch{};
                      });
    if (r.rc != MMT_OK) return r.rc;
    r.flush();
    // bf16 copy for the FFN backward of the modalities no fused epilogue covered
    DropCopyBatch db{}; db.count = 0;
    for (int i = 0; i < M; ++i) {
      if (fuse_copy && last_writer[i] >= 0) continue;
      DropCopyProblem& q = db.p[db.count++];
      q.src = r.f32(p.dres[i]); q.dst = d16_cur(c, r, i); q.dsum = grads + x[i].bf2;
      r.set_drop(q, l, i, DS_FFN);
    }
    r.det_arm(db);
    if (db.count) r.ok(mmt_launch_drop_copy(db, R, C, r.s), "dres16");
  }
  if (r.rc != MMT_OK) return r.rc;
  // FFN: dres16[i] carries the FFN dropout mask; the FFN output-bias grad was summed with it
  const int ffn_dw_hint = kn.dw_attn_small ? 2 : 0;  // (Knobs: MMT_DW_ATTN_SMALL)
  r.dwgemm(gemms(M, [&](int i) { return dw_of(d16_cur(c, r, i), C, a[i].f, 4 * C, x[i].F2); }), "ffn2_dw", ffn_dw_hint);
  r.gemm(gemms(M, [&](int i) {
           GemmProblem d = dx_act(d16_cur(c, r, i), C, x[i].F2, a[i].f, p.gbig[par][i], 4 * C, x[i].bf0);
           if (c->relu_bits) { d.mask8 = r.W<uint8_t>(a[i].fm); d.ldm8 = 4 * C / 8; }  // ReLU' from bits
           return d;
         }), true, false, EPI_DRELU_BF16, 1, "ffn2_dx");
  r.dwgemm(gemms(M, [&](int i) { return dw_of(r.b16(p.gbig[par][i]), 4 * C, a[i].c, C, x[i].F0); }), "ffn0_dw", ffn_dw_hint);
  r.flush();
  d16_advance(c);
  r.gemm_ln_bwd(gemms(M, [&](int i) { return dx_ln(r.b16(p.gbig[par][i]), 4 * C, x[i].F0, i); }),
                lns(M, [&](int i) {
                  LnProblem q = ln_bwd(LN2, i, r.f32(a[i].x1));
                  q.dx16 = d16_cur(c, r, i);
                  r.set_drop(q, l, i, DS_SA_PROJ);  // the copy feeds the SA projection backward
                  q.dsum = grads + x[i].bp2;
                  return q;
                }), R, C, "ffn0_dx", "ln2_bwd");
  // SA output projection
  static const char* const sa_labels[5] = {"proj2_dw", "proj_dx", "proj2_dx", "proj0_dw", "proj0_dx"};
  proj_bwd(M, [](int u) { return u; }, [&](int i) { return ProjMats{&x[i].P0, &x[i].P2, x[i].bp0}; }, &ActLM::p1, &ActLM::o, p.gp,
           sa_labels);
  AttnBatch ab = batch_of<AttnBatch>(M, [&](int i) {
    AttnProblem q = r.self_attn(a[i], l, i);
    bf16_t* gq = r.b16(p.gqkv[i]);
    q.dout = r.b16(p.gdo[i]); q.dout_ld = C; q.dvec[0] = r.f32(p.dvec[i][0]);
    q.dq = gq + C; q.dq_ld = 3 * C; q.dk[0] = gq; q.dv[0] = gq + 2 * C; q.dkv_ld = 3 * C; q.dkv_hstride = hs;
    return q;
  });
  // hs 32: the Q/K/V stage-2 backward runs in the attention kernel's epilogue (dQ / dK / dV stay on chip:
  // dh1, dW2, db1 leave it), so the separate qkv2 backward and its gqkv round trip go
  const bool q2 = kn.attn_qkv2 && mmt_attn_bwd_fuses_qkv2(ab, r.B, T, H, hs);
  if (q2)
    for (int i = 0; i < M; ++i) {
      AttnProblem& q = ab.p[i];
      q.q2_h1 = r.b16(a[i].h1); q.q2_dh1 = r.b16(p.gh1[par][i]); q.q2_ld = ldh1;
      q.q2_w2 = r.P(x[i].w2); q.q2_dw2 = grads + x[i].w2; q.q2_db1 = grads + x[i].b1;
      // Q / K / V on chip, as the forward latched it (bit 1: this kernel makes them from h1 and W2)
      if (c->onchip & 2) { q.oc_h1 = q.q2_h1; q.oc_ld = ldh1; q.oc_w2 = q.q2_w2; }
    }
  if (c->onchip == 3 && !q2)  // (the knobs the forward decided on were changed since)
    return fail(c, MMT_ERR_STATE, "mmt_backward: the forward kept Q/K/V on chip (mmt_set_attn_qkv_onchip) and the "
                                  "backward that makes them again (mmt_set_attn_qkv2, mmt_attn_set_ring bit 6) is off");
  // dh1 rows are padded to ldh1 (a multiple of 8) and the qkv2 backward writes only the 3 H hh columns;
  // the stage-1 dX GEMM reads K in 8-column chunks against zero weight-pack pad rows, so the pad must be
  // finite: zeroed once per workspace (no kernel writes it). Garbage there made the gradient NaN at
  // shapes with 3 H hh % 8 != 0 (hs 8 / 24 with odd head counts; round 6)
  if (p.gh1_pad_ws != r.ws && ldh1 > 3 * H * c->hh) {
    const size_t cols = 3 * (size_t)H * c->hh;
    for (int k = 0; k < 2; ++k)
      for (int i = 0; i < M; ++i)
        r.ok(hipMemset2DAsync(r.b16(p.gh1[k][i]) + cols, (size_t)ldh1 * 2, 0, ((size_t)ldh1 - cols) * 2, (size_t)R, r.s),
             "gh1 pad");
    p.gh1_pad_ws = r.ws;
  }
  r.attn(ab, true, scale, "attn_bwd");
  if (!q2) {
    Qkv2Batch qb{}; qb.count = M;
    for (int i = 0; i < M; ++i) {
      qb.p[i].h1 = r.b16(a[i].h1); qb.p[i].w2 = r.P(x[i].w2); qb.p[i].dout = r.b16(p.gqkv[i]);
      qb.p[i].dh1 = r.b16(p.gh1[par][i]); qb.p[i].dw2 = grads + x[i].w2;
      qb.p[i].db1 = grads + x[i].b1;  // stage-1 bias gradient: column sums of dh1, fused
    }
    r.det_arm(qb);
    r.ok(mmt_launch_qkv2_bwd(qb, R, 3 * H, hs, ldh1, 3 * C, r.s), "qkv2_bwd");
  }
  r.dwgemm(gemms(M, [&](int i) { return dw_of(r.b16(p.gh1[par][i]), ldh1, a[i].a, C, x[i].W1); }), "qkv1_dw");
  r.flush();
  d16_advance(c);
  r.gemm_ln_bwd(gemms(M, [&](int i) { return dx_ln(r.b16(p.gh1[par][i]), ldh1, x[i].W1, i); }),
                lns(M, [&](int i) {
                  LnProblem q = ln_bwd(LN1, i, xin[i]);
                  set_dres16_consumer(c, r, q, i, l - 1, grads);
                  return q;
                }), R, C, "qkv1_dx", "ln1_bwd");
  return r.rc;
}

int check_cfg(const mmt_config* cfg, std::string& msg) {
  if (!cfg) { msg = "null config"; return MMT_ERR_INVALID; }
  const int M = cfg->num_modalities;
  if (M < 1 || M > MAXM) { msg = "num_modalities must be 1..8"; return MMT_ERR_INVALID; }
  if (cfg->n_embd <= 0 || cfg->n_head <= 0 || cfg->n_layer < 0 || cfg->block_size <= 0) {
    msg = "n_embd, n_head, block_size must be positive and n_layer >= 0"; return MMT_ERR_INVALID;
  }
  if (cfg->n_embd % cfg->n_head) { msg = "n_embd must be divisible by n_head"; return MMT_ERR_UNSUPPORTED; }
  const int hs = cfg->n_embd / cfg->n_head;
  if (!(hs == 8 || hs == 16 || hs == 24 || hs == 32 || hs == 48 || hs == 64)) {
    msg = "head size n_embd/n_head must be one of 8,16,24,32,48,64 (got " + std::to_string(hs) + ")";
    return MMT_ERR_UNSUPPORTED;
  }
  if (cfg->n_embd % 8 || cfg->n_embd > 1024) { msg = "n_embd must be a multiple of 8 and <= 1024"; return MMT_ERR_UNSUPPORTED; }
  for (int i = 0; i < M; ++i)
    if (cfg->vocab_sizes[i] < 1) { msg = "vocab sizes must be >= 1"; return MMT_ERR_INVALID; }
  if (cfg->dropout < 0.f || cfg->dropout >= 1.f) { msg = "dropout must be in [0, 1)"; return MMT_ERR_INVALID; }
  if (cfg->precision != 0 && cfg->precision != 1) { msg = "precision must be 0 (bf16) or 1 (fp8)"; return MMT_ERR_INVALID; }
  if (cfg->precision == 1 && cfg->n_embd % 32) {
    msg = "precision fp8 needs n_embd % 32 == 0 (MX blocks of 32 along every fp8 GEMM's K)"; return MMT_ERR_UNSUPPORTED;
  }
  return MMT_OK;
}

int ensure_device_tables(mmt_ctx* c) {
  // the pack tables live on the device of the caller's current stream (rebuilt when the
  // model moves to another device)
  int dev = -1;
  HIPCHK(c, hipGetDevice(&dev));
  if (c->d_segs && c->tables_device == dev) return MMT_OK;
  if (c->d_segs) { (void)hipFree(c->d_segs); c->d_segs = nullptr; }
  if (c->d_tasks) { (void)hipFree(c->d_tasks); c->d_tasks = nullptr; }
  if (c->d_mxsegs) { (void)hipFree(c->d_mxsegs); c->d_mxsegs = nullptr; }
  if (c->segs.empty()) return MMT_OK;
  HIPCHK(c, hipMalloc(&c->d_segs, sizeof(PackSeg) * c->segs.size()));
  HIPCHK(c, hipMalloc(&c->d_tasks, sizeof(int) * c->tasks.size()));
  HIPCHK(c, hipMemcpy(c->d_segs, c->segs.data(), sizeof(PackSeg) * c->segs.size(), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->d_tasks, c->tasks.data(), sizeof(int) * c->tasks.size(), hipMemcpyHostToDevice));
  if (!c->mxsegs.empty()) {
    HIPCHK(c, hipMalloc(&c->d_mxsegs, sizeof(MxSeg) * c->mxsegs.size()));
    HIPCHK(c, hipMemcpy(c->d_mxsegs, c->mxsegs.data(), sizeof(MxSeg) * c->mxsegs.size(), hipMemcpyHostToDevice));
  }
  c->tables_device = dev;
  return MMT_OK;
}

// the side stream (weight-gradient GEMMs in the backward, dropout keep bits in the forward), made
// lazily on the caller's current device (Knobs: MMT_SIDE_STREAM, MMT_SIDE_PRIORITY)
void ensure_side(mmt_ctx* c) {
  int dev = -1;
  if (knobs().side_stream == 0 || hipGetDevice(&dev) != hipSuccess || (c->side && c->side_device == dev)) return;
  if (c->side) (void)hipStreamDestroy(c->side);
  for (auto& e : c->evpool) (void)hipEventDestroy(e);  // events of the previous device
  c->evpool.clear();
  c->side = nullptr;
  const char* prio_env = knobs().side_priority;
  // (a CU-masked side stream measured far slower -- it cannot be created non-blocking, so it
  // serialises against the caller's stream: profiles/r3q_side_cumask_ab.txt; removed in round 4)
  hipError_t ce;
  if (prio_env) {
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    const int pr = std::max(greatest, std::min(least, atoi(prio_env)));
    ce = hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, pr);
  } else {
    ce = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
  }
  if (ce != hipSuccess) c->side = nullptr;
  c->side_device = dev;
  while (c->side && c->evpool.size() < 64) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) break;
    c->evpool.push_back(e);
  }
  for (auto& e : c->stage_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
    if (c->side && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
  }
  if ((c->evpool.empty() || !c->stage_ev[0] || !c->stage_ev[1]) && c->side) {
    (void)hipStreamDestroy(c->side);
    c->side = nullptr;
  }
}

}  // namespace

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

const char* mmt_version(void) { return "mmt_hip 0.2 gfx950"; }
const char* mmt_create_error(void) { return g_create_err.c_str(); }

mmt_ctx* mmt_create(const mmt_config* cfg) {
  std::string msg;
  if (check_cfg(cfg, msg) != MMT_OK) { g_create_err = msg; return nullptr; }
  mmt_ctx* c = new (std::nothrow) mmt_ctx();
  if (!c) { g_create_err = "out of memory"; return nullptr; }
  c->cfg = *cfg;
  c->M = cfg->num_modalities; c->C = cfg->n_embd; c->H = cfg->n_head; c->L = cfg->n_layer; c->T = cfg->block_size;
  c->hs = c->C / c->H; c->hh = c->hs / 2;
  for (int i = 0; i < c->M; ++i) {
    c->V[i] = cfg->vocab_sizes[i];
    if (cfg->cross_attention[i] && c->M > 1) { c->any_cross = true; ++c->ncross; }
  }
  if (c->M - 1 > MMT_MAX_STREAMS) { g_create_err = "too many KV streams"; delete c; return nullptr; }
  c->fp8 = cfg->precision == 1;
  c->relu_bits = knobs().relu_bits != 0;
  build_layout(c);
  return c;
}

void mmt_destroy(mmt_ctx* c) {
  if (!c) return;
  if (c->d_segs) (void)hipFree(c->d_segs);
  if (c->d_tasks) (void)hipFree(c->d_tasks);
  if (c->d_mxsegs) (void)hipFree(c->d_mxsegs);
  for (auto& e : c->probe_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  for (auto& e : c->evpool) (void)hipEventDestroy(e);
  for (auto& e : c->stage_ev) if (e) (void)hipEventDestroy(e);
  if (c->emb_ev) (void)hipEventDestroy(c->emb_ev);
  if (c->side) (void)hipStreamDestroy(c->side);
  delete c;
}

const char* mmt_last_error(const mmt_ctx* c) { return c ? c->err.c_str() : "null context"; }
int64_t mmt_param_count(const mmt_ctx* c) { return c ? c->nparams : 0; }
int64_t mmt_param_active_count(const mmt_ctx* c) { return c ? c->nactive : 0; }
int32_t mmt_tensor_count(const mmt_ctx* c) { return c ? (int32_t)c->tensors.size() : 0; }

int mmt_tensor_info(const mmt_ctx* c, int32_t i, char* name, int32_t cap, int64_t* off, int32_t* nd, int64_t* shape,
                    int32_t* kind) {
  if (!c || i < 0 || i >= (int32_t)c->tensors.size()) return MMT_ERR_INVALID;
  const TensorInfo& t = c->tensors[i];
  if (name && cap > 0) {
    std::strncpy(name, t.name.c_str(), cap - 1);
    name[cap - 1] = 0;
  }
  if (off) *off = t.off;
  if (nd) *nd = t.nd;
  if (shape) { shape[0] = t.shape[0]; shape[1] = t.shape[1]; }
  if (kind) *kind = t.kind;
  return MMT_OK;
}

int64_t mmt_loss_flag_offset(mmt_ctx* c, int32_t batch) {
  if (!c || batch < 1) return -1;
  return (int64_t)flag_offset(c);  // batch-independent: the current plan is left alone
}

int64_t mmt_workspace_bytes(mmt_ctx* c, int32_t batch) {
  if (!c || batch < 1) return -1;
  make_plan(c, batch);
  c->last_B = batch;
  c->fwd_ready = false;
  c->cache_ready = false;
  c->fan_next = -1;
  return (int64_t)c->plan.total;
}

int mmt_forward(mmt_ctx* c, void* stream, int32_t batch, const int64_t* const* idx, const int64_t* const* tgt,
                const float* params, float* const* logits, float* losses, void* workspace, int32_t training) {
  if (!c) return MMT_ERR_INVALID;
  if (batch < 1 || !idx || !params || !logits || !workspace) return fail(c, MMT_ERR_INVALID, "mmt_forward: null argument");
  if (c->plan.B != batch) make_plan(c, batch);
  int rc = ensure_device_tables(c);
  if (rc) return rc;
  c->side_off = c->side_off_req;
  c->det = c->det_req;
  c->onchip_req = training ? knobs().attn_qkv_onchip : 0;
  c->onchip = 0;
  Runner r{c, (hipStream_t)stream, workspace, params, nullptr, batch, batch * c->T};
  // dropout (training mode only, as nn.Dropout): one seed per training forward, reused by its backward
  r.drop = training && c->cfg.dropout > 0.f;
  if (r.drop) {
    if (c->next_seed_set) r.seed = c->next_seed;
    else r.seed = ((uint64_t)mmt_hash((uint32_t)c->cfg.seed, (uint32_t)(c->cfg.seed >> 32), (uint32_t)c->step_counter) << 32) |
                  mmt_hash((uint32_t)(c->cfg.seed >> 32), (uint32_t)c->cfg.seed, (uint32_t)(c->step_counter >> 32) ^ 0xA5A5A5A5u);
    c->next_seed_set = false;
    ++c->step_counter;
  }
  if (r.drop) ensure_side(c);
  c->fwd_drop = r.drop;
  c->fwd_seed = r.seed;
  c->fwd_ready = false;
  c->fan_next = -1;  // a new prefill ends a fan-out run
  for (int i = 0; i < c->M; ++i) c->last_idx[i] = idx[i];
  rc = run_forward(c, r, idx, tgt, logits, losses);
  if (rc == MMT_OK && tgt) c->fwd_ready = true;
  c->cache_ready = rc == MMT_OK;  // the saved Q/K/V of this forward serve mmt_decode_step
  c->last_training = training != 0;
  return rc;
}

int mmt_decode_step(mmt_ctx* c, void* stream, int32_t batch, int32_t pos, const int64_t* const* idx,
                    const float* params, float* const* logits, void* workspace) {
  if (!c) return MMT_ERR_INVALID;
  if (!idx || !params || !logits || !workspace) return fail(c, MMT_ERR_INVALID, "mmt_decode_step: null argument");
  if (c->plan.B != batch || !c->cache_ready)
    return fail(c, MMT_ERR_STATE, "mmt_decode_step: run mmt_forward (prefill) on this batch and workspace first");
  if (c->onchip == 3)
    return fail(c, MMT_ERR_INVALID, "mmt_decode_step: the last forward (training != 0) kept the self-attention Q/K/V on "
                                    "chip (mmt_set_attn_qkv_onchip), so the workspace holds no K/V cache: run the "
                                    "prefill with training = 0");
  if (c->fwd_drop)
    return fail(c, MMT_ERR_STATE, "mmt_decode_step: the prefill forward sampled dropout (training mode); decode "
                                  "has eval semantics: run the prefill with training = 0");
  if (c->fp8)
    return fail(c, MMT_ERR_STATE, "mmt_decode_step: precision fp8 prefills with MX-fp8 GEMMs the bf16 decode "
                                  "would not reproduce: re-run mmt_forward per token");
  if (pos < 1 || pos >= c->T) return fail(c, MMT_ERR_INVALID, "mmt_decode_step: position outside 1..block_size-1");
  Runner r{c, (hipStream_t)stream, workspace, params, nullptr, batch, batch};
  const DecWhere w{static_cast<char*>(workspace), c->plan.dec, c->plan.dec_x.data(), batch};
  return run_decode(c, r, w, pos, idx, logits);
}

int64_t mmt_fanout_bytes(mmt_ctx* c, int32_t batch, int32_t samples, int32_t max_new) {
  if (!c) return -1;
  FanPlan f;
  if (!make_fan_plan(c, f, batch, samples, max_new)) return -1;
  return (int64_t)f.total;
}

int mmt_decode_fanout_step(mmt_ctx* c, void* stream, int32_t batch, int32_t samples, int32_t n0, int32_t max_new,
                           int32_t pos, const int64_t* const* idx, const float* params, float* const* logits,
                           const void* workspace, void* fan) {
  if (!c) return MMT_ERR_INVALID;
  const char* me = "mmt_decode_fanout_step";
  if (!idx || !params || !logits || !workspace || !fan) return fail(c, MMT_ERR_INVALID, std::string(me) + ": null argument");
  if (c->plan.B != batch || !c->cache_ready)
    return fail(c, MMT_ERR_STATE, std::string(me) + ": run mmt_forward (prefill) on this batch and workspace first");
  if (c->onchip == 3)
    return fail(c, MMT_ERR_INVALID, std::string(me) + ": the last forward (training != 0) kept the self-attention Q/K/V "
                                    "on chip, so the workspace holds no K/V cache: run the prefill with training = 0");
  if (c->fwd_drop)
    return fail(c, MMT_ERR_STATE, std::string(me) + ": the prefill forward sampled dropout (training mode); decode has "
                                  "eval semantics: run the prefill with training = 0");
  if (c->fp8)
    return fail(c, MMT_ERR_STATE, std::string(me) + ": precision fp8 prefills with MX-fp8 GEMMs the bf16 decode would "
                                  "not reproduce");
  if (samples < 1 || n0 < 1 || max_new < 1 || (int64_t)n0 + max_new > c->T)
    return fail(c, MMT_ERR_INVALID, std::string(me) + ": need samples >= 1, n0 >= 1, max_new >= 1, n0 + max_new <= block_size");
  if (pos < n0 || pos >= n0 + max_new) return fail(c, MMT_ERR_INVALID, std::string(me) + ": position outside n0..n0+max_new-1");
  const bool same = c->fan.B == batch && c->fan.S == samples && c->fan.max_new == max_new;
  if (pos != n0 && (!same || c->fan_next != pos || c->fan_n0 != n0 || c->fan_S != samples))
    return fail(c, MMT_ERR_STATE, std::string(me) + ": a run starts at pos == n0 and continues one position at a time "
                                  "with the same batch, samples, n0 and max_new");
  if (!same) {  // a run with another buffer shape starts
    FanPlan f;
    if (!make_fan_plan(c, f, batch, samples, max_new))
      return fail(c, MMT_ERR_INVALID, std::string(me) + ": batch * samples rows exceed the launchers' range");
    c->fan = std::move(f);
  }
  c->fan_next = -1;
  Runner r{c, (hipStream_t)stream, const_cast<void*>(workspace), params, nullptr, batch, batch * samples};
  DecWhere w{static_cast<char*>(fan), c->fan.dec, c->fan.dec_x.data(), batch * samples};
  w.fan = &c->fan; w.S = samples; w.n0 = n0;
  const int rc = run_decode(c, r, w, pos, idx, logits);
  if (rc == MMT_OK) { c->fan_n0 = n0; c->fan_S = samples; c->fan_next = pos + 1; }
  return rc;
}

int64_t mmt_rolling_bytes(mmt_ctx* c, int32_t batch, int32_t samples, int32_t max_tail) {
  if (!c) return -1;
  RollPlan f;
  if (!make_roll_plan(c, f, batch, samples, max_tail)) return -1;
  return (int64_t)f.total;
}

int mmt_rolling_step(mmt_ctx* c, void* stream, int32_t batch, int32_t samples, int32_t p, int32_t m,
                     const int64_t* const* idx, int64_t idx_ld, const float* params, float* const* logits,
                     const void* workspace, void* roll) {
  if (!c) return MMT_ERR_INVALID;
  const char* me = "mmt_rolling_step";
  if (!idx || !params || !logits || !workspace || !roll) return fail(c, MMT_ERR_INVALID, std::string(me) + ": null argument");
  for (int i = 0; i < c->M; ++i)
    if (!idx[i] || !logits[i]) return fail(c, MMT_ERR_INVALID, std::string(me) + ": null token or logits pointer");
  if (batch < 1) return fail(c, MMT_ERR_INVALID, std::string(me) + ": need batch >= 1");
  if (c->plan.B != batch || !c->cache_ready)
    return fail(c, MMT_ERR_STATE, std::string(me) + ": run mmt_forward over the prefix on this batch and workspace first");
  if (c->onchip == 3)
    return fail(c, MMT_ERR_INVALID, std::string(me) + ": the last forward (training != 0) kept the self-attention Q/K/V "
                                    "on chip, so the workspace holds no K/V cache: run the forward with training = 0");
  if (c->fwd_drop)
    return fail(c, MMT_ERR_STATE, std::string(me) + ": the forward sampled dropout (training mode); the step has eval "
                                  "semantics: run the forward with training = 0");
  if (c->fp8)
    return fail(c, MMT_ERR_STATE, std::string(me) + ": precision fp8 runs the forward with MX-fp8 GEMMs the bf16 step "
                                  "would not reproduce");
  if (samples < 1 || p < 1 || m < 1 || (int64_t)p + m > c->T || idx_ld < m)
    return fail(c, MMT_ERR_INVALID, std::string(me) + ": need samples >= 1, p >= 1, m >= 1, p + m <= block_size, "
                                    "idx_ld >= m");
  // the plan of exactly m tail rows: no state is kept, and a buffer of mmt_rolling_bytes(max_tail >= m) holds it
  RollPlan f;
  if (!make_roll_plan(c, f, batch, samples, m))
    return fail(c, MMT_ERR_INVALID, std::string(me) + ": batch * samples * m rows exceed the launchers' range");
  const int rows = batch * samples * m;
  Runner r{c, (hipStream_t)stream, const_cast<void*>(workspace), params, nullptr, batch, rows};
  DecWhere w{static_cast<char*>(roll), f.dec, f.dec_x.data(), rows};
  w.S = samples; w.xlayers = 2; w.roll_p = p; w.roll_m = m; w.idx_ld = idx_ld; w.last = f.last;
  return run_decode(c, r, w, p, idx, logits);
}

int mmt_fanout_gather(mmt_ctx* c, void* stream, int32_t batch, int32_t samples, int32_t n0, int32_t max_new,
                      int32_t npos, const int32_t* ancestors, const void* src_fan, void* dst_fan) {
  if (!c) return MMT_ERR_INVALID;
  const char* me = "mmt_fanout_gather";
  if (!ancestors || !src_fan || !dst_fan) return fail(c, MMT_ERR_INVALID, std::string(me) + ": null argument");
  if (src_fan == dst_fan) return fail(c, MMT_ERR_INVALID, std::string(me) + ": src_fan and dst_fan are one buffer");
  if (c->fan_next < 0 || c->fan.B != batch || c->fan.S != samples || c->fan.max_new != max_new || c->fan_n0 != n0 ||
      c->fan_S != samples)
    return fail(c, MMT_ERR_STATE, std::string(me) + ": batch, samples, n0 and max_new must be those of the fan-out run "
                                  "in progress");
  if (npos != c->fan_next - n0)
    return fail(c, MMT_ERR_INVALID, std::string(me) + ": npos must be the number of positions the run has written");
  if ((((uintptr_t)src_fan | (uintptr_t)dst_fan) & 15) != 0)
    return fail(c, MMT_ERR_INVALID, std::string(me) + ": fan buffers must be 16-byte aligned");
  // the segment table is the plan's: every self-attention and cross tail, rows max_new * ld elements apart, the
  // first npos positions of each (contiguous in a row); the compact per-step scratch in front is not copied
  const FanPlan& f = c->fan;
  const int M = c->M, C = c->C;
  const int rows = batch * samples;
  const char* src = static_cast<const char*>(src_fan);
  char* dst = static_cast<char*>(dst_fan);
  hipStream_t s = (hipStream_t)stream;
  GatherBatch gb{};
  auto flush = [&]() -> bool {
    if (gb.count == 0) return true;
    const hipError_t e = mmt_launch_row_gather(gb, ancestors, rows, s);
    gb.count = 0;
    return e == hipSuccess;
  };
  auto add = [&](size_t off, int ld) -> bool {
    GatherSeg& q = gb.seg[gb.count++];
    q.src = src + off; q.dst = dst + off;
    q.row_bytes = (int64_t)max_new * ld * 2; q.bytes = (int64_t)npos * ld * 2;
    return gb.count < MMT_GATHER_SEGS || flush();
  };
  bool ok = true;
  for (int l = 0; l < c->L && ok; ++l)
    for (int i = 0; i < M && ok; ++i) {
      ok = add(f.sa_tail[(size_t)l * M + i], 3 * C);
      if (c->lm[(size_t)l * M + i].cross)
        for (int j = 0; j < M - 1 && ok; ++j) ok = add(f.ca_tail[((size_t)l * M + i) * MAXM + j], 2 * C);
    }
  ok = ok && flush();
  return ok ? MMT_OK : fail(c, MMT_ERR_HIP, std::string(me) + ": launch failed");
}

int32_t mmt_backward_stage_count(const mmt_ctx* c) { return c ? c->L + 2 : 0; }

int mmt_backward_stage_range(const mmt_ctx* c, int32_t stage, int64_t* begin, int64_t* end) {
  if (!c || stage < 0 || stage > c->L + 1) return MMT_ERR_INVALID;
  int64_t b, e;
  if (stage == 0) { b = c->post_begin; e = c->post_end; }
  else if (stage == c->L + 1) { b = c->emb_begin; e = c->emb_end; }
  else { const int l = c->L - stage; b = c->layer_begin[l]; e = c->layer_end[l]; }
  if (begin) *begin = b;
  if (end) *end = e;
  return MMT_OK;
}

}  // extern "C"

extern "C" {

int mmt_backward_stage(mmt_ctx* c, void* stream, int32_t stage, const float* loss_grads, const float* params,
                       float* grads, void* workspace) {
  if (!c) return MMT_ERR_INVALID;
  if (!c->fwd_ready) return fail(c, MMT_ERR_STATE, "mmt_backward: no forward with targets to differentiate");
  if (stage < 0 || stage > c->L + 1) return fail(c, MMT_ERR_INVALID, "bad backward stage");
  ensure_side(c);
  Runner r{c, (hipStream_t)stream, workspace, params, nullptr, c->plan.B, c->plan.B * c->T};
  r.drop = c->fwd_drop;
  r.seed = c->fwd_seed;
  r.det = c->det;
  if (c->det && stage == 0) {
    // the token-table gradient has a fixed summation order only through the stable row sort: outside its
    // limits the step is refused here, before anything is launched, never run in arrival order
    EmbBatch eb{}; eb.count = c->M;
    for (int i = 0; i < c->M; ++i) { eb.p[i].V = c->V[i]; eb.p[i].perm = r.W<int>(c->plan.eperm[i]); }
    if (!mmt_embed_bwd_det_ok(eb, r.R, c->C))
      return fail(c, MMT_ERR_UNSUPPORTED,
                  "deterministic mode: the token-table gradient's stable row sort covers batch * block_size <= 16384 "
                  "rows, vocabularies <= 16384 and n_embd <= 1024 (with MMT_EMB_SORT on); got " +
                      std::to_string(r.R) + " rows");
  }
  if (stage == c->L + 1) {
    EmbBatch eb{}; eb.count = c->M;
    for (int i = 0; i < c->M; ++i) {
      eb.p[i].idx = c->last_idx[i]; eb.p[i].dx = r.W<float>(c->plan.dres[i]);
      eb.p[i].dtok = grads + c->post[i].tok; eb.p[i].dpos = grads + c->pos_off; eb.p[i].V = c->V[i];
      eb.p[i].part = r.W<float>(c->plan.dln[i]);  // R x C fp32, free once the layers are done
      if (c->emb_sorted) eb.p[i].perm = r.W<int>(c->plan.eperm[i]);  // sorted at stage 0
    }
    if (c->emb_sorted) r.ok(hipStreamWaitEvent(r.s, c->emb_ev, 0), "stream wait");
    c->emb_sorted = false;
    r.det_arm(eb);
    r.ok(mmt_launch_embed_bwd(eb, r.B, c->T, c->C, r.s), "embed_bwd");
    return r.rc;
  }
  const bool defer = c->defer_join && r.side_stream();
  if (defer && stage >= 2)  // the side stream's work of stage - 2 read this stage's scratch copies
    r.ok(hipStreamWaitEvent(r.s, c->stage_ev[stage & 1], 0), "stream wait");
  r.hold = defer && knobs().flush_hold && stage < c->L;  // (Knobs: MMT_FLUSH_HOLD)
  const int rc = run_backward_stage(c, r, stage, loss_grads, grads);
  r.hold = false;
  if (defer) {
    r.flush(true);
    r.ok(hipEventRecord(c->stage_ev[stage & 1], c->side), "event record");
  } else {
    r.join();  // the stage's gradient range is complete on the caller's stream (DP all-reduce order)
  }
  return rc ? rc : r.rc;
}

int mmt_backward(mmt_ctx* c, void* stream, const float* loss_grads, const float* params, float* grads,
                 void* workspace) {
  if (!c) return MMT_ERR_INVALID;
  // one join at the end instead of one per stage (mmt_ctx::defer_join); the embedding stage is the
  // last and runs on the caller's stream only, so the join closes over every weight gradient
  c->defer_join = true;
  int rc = MMT_OK;
  for (int s = 0; s < c->L + 2 && rc == MMT_OK; ++s) rc = mmt_backward_stage(c, stream, s, loss_grads, params, grads, workspace);
  c->defer_join = false;
  // the join also on the error path: no weight-gradient GEMM (or its split-K slab) of this backward is
  // left running on the side stream once control is back with the caller
  Runner r{c, (hipStream_t)stream, workspace, params, nullptr, c->plan.B, c->plan.B * c->T};
  r.join();
  return rc ? rc : r.rc;
}

int mmt_adamw_step(mmt_ctx* c, void* stream, float* params, const float* grads, float* m, float* v, int64_t n,
                   int64_t step, float lr, float b1, float b2, float eps, float wd) {
  if (step < 1 || !params || !grads || !m || !v) return fail(c, MMT_ERR_INVALID, "mmt_adamw_step: bad argument");
  const double bc1 = 1.0 - std::pow((double)b1, (double)step);
  const double bc2 = 1.0 - std::pow((double)b2, (double)step);
  const hipError_t e = mmt_launch_adamw(params, grads, m, v, n, lr, b1, b2, eps, wd, (float)bc1,
                                        (float)std::sqrt(bc2), (hipStream_t)stream);
  if (e != hipSuccess) return fail(c, MMT_ERR_HIP, std::string("adamw: ") + hipGetErrorString(e));
  return MMT_OK;
}

int64_t mmt_guard_state_bytes(void) {
  return (int64_t)sizeof(mmt_guard_header) + (int64_t)MMT_GUARD_SLOTS * (int64_t)sizeof(double);
}

static bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

int mmt_grad_sqsum(void* stream, const float* grads, int64_t n, int32_t add, void* guard) {
  if (!guard || n < 0 || (n > 0 && !grads) || misaligned16(grads) || misaligned16(guard)) return MMT_ERR_INVALID;
  return mmt_launch_grad_sqsum(grads, n, add != 0, guard, (hipStream_t)stream) == hipSuccess ? MMT_OK : MMT_ERR_HIP;
}

int mmt_guard_finalize(void* stream, float max_norm, int32_t skip_nonfinite, float beta1, float beta2, void* guard) {
  if (!guard || misaligned16(guard)) return MMT_ERR_INVALID;
  return mmt_launch_guard_finalize(guard, max_norm, skip_nonfinite != 0, beta1, beta2, (hipStream_t)stream) == hipSuccess
             ? MMT_OK
             : MMT_ERR_HIP;
}

int mmt_adamw_step_guarded(mmt_ctx* c, void* stream, float* params, const float* grads, float* m, float* v, int64_t n,
                           float lr, float b1, float b2, float eps, float wd, const void* guard) {
  if (!guard || n < 0 || !params || !grads || !m || !v)
    return fail(c, MMT_ERR_INVALID, "mmt_adamw_step_guarded: bad argument");
  if (misaligned16(params) || misaligned16(grads) || misaligned16(m) || misaligned16(v) || misaligned16(guard))
    return fail(c, MMT_ERR_INVALID, "mmt_adamw_step_guarded: pointers must be 16-byte aligned");
  const hipError_t e = mmt_launch_adamw_guarded(params, grads, m, v, n, lr, b1, b2, eps, wd, guard, (hipStream_t)stream);
  if (e != hipSuccess) return fail(c, MMT_ERR_HIP, std::string("adamw_guarded: ") + hipGetErrorString(e));
  return MMT_OK;
}

int mmt_eval_direction(mmt_ctx* c, void* stream, int32_t batch, int32_t T, int32_t V, const float* logits,
                       const int64_t* xb, const int64_t* yb, const double* vocab, int32_t is_percent,
                       int32_t* wins_losses, double* certainty_sum) {
  const hipError_t e = mmt_launch_eval_direction(logits, xb, yb, vocab, batch, T, V, is_percent, wins_losses,
                                                 certainty_sum, (hipStream_t)stream);
  if (e != hipSuccess) return fail(c, MMT_ERR_HIP, std::string("eval_direction: ") + hipGetErrorString(e));
  return MMT_OK;
}

}  // extern "C"


// seed of the dropout masks of the next training forward (and its backward); without a call the
// engine derives one from mmt_config.seed and a per-context counter
extern "C" int mmt_set_dropout_seed(mmt_ctx* c, uint64_t seed) {
  if (!c) return MMT_ERR_INVALID;
  c->next_seed = seed;
  c->next_seed_set = true;
  return MMT_OK;
}

// live per-kernel timing: HIP events around every launch whose label matches one of the
// comma-separated patterns of `label` (e.g. "*_dw,attn_fwd,attn_bwd,ffn0"), recorded on the stream
// the launch runs on, so bench.py can price kernels inside the timed region.
// serial mode for measurement (bench.py's serial roofline leg): 0 = everything of this context on the
// caller's stream, 1 = the side stream again. Latched: the next mmt_forward applies it, so a call between
// a forward and its backward (or between backward stages) never strands forked side-stream work
extern "C" int mmt_set_side_stream(mmt_ctx* c, int32_t on) {
  if (!c) return MMT_ERR_INVALID;
  c->side_off_req = on == 0;
  return MMT_OK;
}

// deterministic mode (mmt.h): latched like the side-stream switch, per context
extern "C" int mmt_set_deterministic(mmt_ctx* c, int32_t on) {
  if (!c) return MMT_ERR_INVALID;
  c->det_req = on != 0;
  return MMT_OK;
}
extern "C" int32_t mmt_get_deterministic(const mmt_ctx* c) { return c && c->det_req ? 1 : 0; }

// the training objective (include/mmt.h): checked in full before anything is stored
extern "C" int mmt_set_loss(mmt_ctx* c, const mmt_loss_spec* spec) {
  if (!c) return MMT_ERR_INVALID;
  bool on = false;
  for (int i = 0; spec && i < c->M; ++i) {
    const float e = spec[i].label_smoothing;
    if (!(e >= 0.f && e < 1.f)) return fail(c, MMT_ERR_INVALID, "mmt_set_loss: label_smoothing outside [0, 1)");
    on = on || e != 0.f || spec[i].class_weight || spec[i].position_weight;
  }
  for (int i = 0; i < MAXM; ++i) c->loss[i] = (spec && i < c->M) ? spec[i] : mmt_loss_spec{};
  c->loss_on = on;
  return MMT_OK;
}
extern "C" int mmt_get_loss(const mmt_ctx* c, mmt_loss_spec* out) {
  if (!c || !out) return MMT_ERR_INVALID;
  for (int i = 0; i < c->M; ++i) out[i] = c->loss[i];
  return MMT_OK;
}

// in-place gradient accumulation (mmt.h): read at stage 0 of the backward, per context
extern "C" int mmt_set_grad_accumulate(mmt_ctx* c, int32_t on) {
  if (!c) return MMT_ERR_INVALID;
  c->grad_accum = on != 0;
  return MMT_OK;
}
extern "C" int32_t mmt_get_grad_accumulate(const mmt_ctx* c) { return c && c->grad_accum ? 1 : 0; }

extern "C" int mmt_probe_set(mmt_ctx* c, const char* label) {
  if (!c) return MMT_ERR_INVALID;
  c->probe_events.clear();
  c->probe_pats.clear();
  if (label) {
    std::string cur;
    for (const char* q = label;; ++q) {
      if (*q == ',' || *q == 0) {
        if (!cur.empty()) c->probe_pats.push_back(cur);
        cur.clear();
        if (!*q) break;
      } else if (*q != ' ') {
        cur += *q;
      }
    }
  }
  // event pairs for the recorded launches, made here (event creation is a host call of tens of
  // microseconds: inside the timed loop it starved the GPU); recording stops when they run out
  const size_t pool = (size_t)knobs().probe_events;
  while (!c->probe_pats.empty() && c->probe_pool.size() < pool) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) break;
    if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); break; }
    c->probe_pool.push_back({a, b});
  }
  return MMT_OK;
}

extern "C" int mmt_probe_enable(mmt_ctx* c, int32_t on) {
  if (!c) return MMT_ERR_INVALID;
  c->probe_on = on != 0;
  return MMT_OK;
}

extern "C" int32_t mmt_probe_count(const mmt_ctx* c) { return c ? (int32_t)c->probe_pats.size() : 0; }

extern "C" int mmt_probe_read_at(mmt_ctx* c, int32_t pat, double* total_ms, int64_t* launches, double* flops,
                                 double* bytes) {
  if (!c) return MMT_ERR_INVALID;
  double tot = 0.0, fl = 0.0, by = 0.0;
  int64_t n = 0;
  for (auto& e : c->probe_events) {
    if (pat >= 0 && e.pat != pat) continue;
    float ms = 0.f;
    if (hipEventSynchronize(e.b) != hipSuccess) return fail(c, MMT_ERR_HIP, "probe event sync");
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) return fail(c, MMT_ERR_HIP, "probe elapsed");
    tot += ms;
    fl += e.flops;
    by += e.bytes;
    ++n;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = n;
  if (flops) *flops = fl;
  if (bytes) *bytes = by;
  return MMT_OK;
}

extern "C" int mmt_probe_read(mmt_ctx* c, double* total_ms, int64_t* launches) {
  return mmt_probe_read_at(c, -1, total_ms, launches, nullptr, nullptr);
}
