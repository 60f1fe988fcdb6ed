// net.cpp -- native runtime of the two networks built by models/model_utilities.lua:
//   create_proposal_net (:3-74)       -> frcnn_pnet_forward / frcnn_pnet_backward
//   create_classification_net (:76-124) -> frcnn_cnet_forward / frcnn_cnet_backward
// The Lua modules own their output/gradInput buffers and reuse them on the next call; so does
// this runtime (all activations, gradient buffers and packed weights live in HBM for the life of
// the model and are re-used every step; nothing is allocated inside a step once shapes settle).
//
// What is stored per convolution is only its PRE-activation output x.  nn.PReLU and
// nn.SpatialDropout are applied by whoever consumes x (the next conv's LDS loader, the pool, the
// weight-gradient loader), and their backward is fused with the pooling backward / bias-gradient
// reduction, so each layer costs one HBM write in forward and one in backward.
//
// Flat parameter order (utilities.lua:136-147): see frcnn_model_param_table.
#include <array>
#include <vector>
#include <cmath>
#include <cstring>
#include <mutex>

#include "kernels.h"
#include "own.h"
#include "linear.h"
#include "pack_tables.h"

namespace frcnn {

static const int HEAD_OUT = 18;  // 3 * (2 + 4), model_utilities.lua:33
static const int SPARSE_MAX_POS = 512;  // above this the dense head backward is used

struct Conv {
  int Cin, Cout, k, pad;
  int H, W, Ho, Wo;           // input / output spatial size (set by ensure_shapes)
  long w_off, b_off, a_off;   // flat offsets; a_off = PReLU slope following this conv (-1: none)
  int block, step;            // backbone position (block -1 for head convs)
  DevBuf wf, wd;              // packed weights (forward / input-gradient)
  DevBuf wx, wxd;             // split-bf16 operand stages (convx.hip) for the launches that take that form
  bool x_f = false, x_d = false;
  DevBuf x, gx;               // pre-activation output and its gradient
  int am = -1;                // first of this convolution's three magnitude records in frcnn_model::amax: |x| (its output), |gx|, |w|
};

struct Block {
  int first_conv, nconv;
  bool has_drop;
  float p_drop;
  DevBuf scale;               // per-channel SpatialDropout scale (mask | 1-p)
  DevBuf pooled, gpooled;
  DevBuf pidx;
  int Hp, Wp;
  int am = -1;                // magnitude record of `pooled`
  // Channels a SpatialDropout keeps (round 6, option "drop_compact"): a block of >= 2 convolutions whose dropout sits behind its
  // first one (models/model_utilities.lua:9-12) is, for the length of one training step, a NARROWER network -- the dropped
  // channels of the first convolution's output are multiplied by zero on the way forward and on the way back, so neither they
  // nor anything computed from them is needed.  With the keep vector known on the host, the step runs the first convolution
  // with the kept filters only (its output, and that output's gradient, are stored COMPACT: kept channels first) and the second
  // one with the kept input channels only; the packs gather the filters / channels, the weight gradients are scattered back.
  // Same results as multiplying by the zeros (sums of exact zeros left out), 25-37 % less matrix work in these layers.
  bool dc_on = false;         // this step runs the block compact
  int nk = 0, nkM = 0, nkK = 0;   // channels kept; padded to a multiple of 64 (a filter / tile dimension) and of 16 (a K dimension)
  const int* dc_idx = nullptr;    // device table of this step: entry i < nk = the i-th kept channel, nk <= i < C: -1
  DevBuf dc_bias;             // the first convolution's bias, gathered (nkM entries, padding 0)
};

struct Head {
  Conv c3;                    // k x k valid conv + PReLU
  Conv c1;                    // 1 x 1 conv -> 18 planes
  int input;                  // 0-based block index
  DevBuf delta;               // delta_outputs[h]
  const int* sp_pos = nullptr; // optional one-shot hint: delta is zero outside these positions
  int sp_count = -1;
  DevBuf spD, spHX, spHY, spGH, spCol, spDX;  // scratch of the sparse backward pass (per anchor net: they run concurrently)
  DevBuf spOut, spSlab;       // sparse training path (heads.hip): the 18 output planes at the sampled positions; K-split partial sums of HX
  hipStream_t stream = nullptr;  // this anchor net's own stream (forward and sparse backward beside the other anchor nets)
  Event done;                    // last work queued on `stream`
  Event gin_done;                // sparse backward: this net's contribution to the pooled map's gradient has been added (the
                                 // backbone's backward pass waits for THIS; the parameter gradients behind it are joined at its end)
  bool gin_recorded = false;
};

struct ClsLayer {
  int in, n;
  bool bn;
  float p_drop;
  long w_off, b_off, bnw_off, bnb_off, a_off;
  DevBuf lin, pre, post, xhat, invstd, mask, g;
  DevBuf gin;                 // gradient wrt this layer's input (layers > 0; a buffer of its own: the weight gradient reads the input beside it)
  Linear fc;                  // the layer's three large products and the operand forms they run in (linear.h)
};

}  // namespace frcnn

using namespace frcnn;

// an on/off switch of the environment (FRCNN_*): unset = dflt, otherwise whether it reads as a non-zero number
static bool env_flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) != 0 : dflt;
}

static int g_drop_compact = -1;   // option "drop_compact" (environment FRCNN_DROP_COMPACT), default on
static int drop_compact_on() {
  if (g_drop_compact < 0) g_drop_compact = env_flag("FRCNN_DROP_COMPACT", true);
  return g_drop_compact;
}
// The library's streams are the PROCESS's, not a model's: the runtime multiplexes every stream onto four hardware queues
// (GPU_MAX_HW_QUEUES; five or more run this step 1.6x slower, tools/r6_hwq.sh), two streams on one queue serialise, and a second
// model with six streams of its own (bench.py's legs, a training and an evaluation model side by side) made both slower.
// Slot 0: the side stream (weight gradients), 1: the classification net's weight gradients / the update stream, 2..6: anchor nets.
static int pool_stream(int slot, hipStream_t* out) {
  static hipStream_t pool[8] = {};
  static std::mutex mu;   // (two host threads may drive two models)
  std::lock_guard<std::mutex> lock(mu);
  if (!pool[slot]) FR_HIP(hipStreamCreateWithFlags(&pool[slot], hipStreamNonBlocking));
  *out = pool[slot];
  return FRCNN_OK;
}

// ---- the anchor nets' sparse training path (heads.hip) ---------------------------------------------------------------------
static int g_sparse_heads = -1;   // option "sparse_heads" (environment FRCNN_SPARSE_HEADS), default on
static int sparse_heads_on() {
  if (g_sparse_heads < 0) g_sparse_heads = env_flag("FRCNN_SPARSE_HEADS", true);
  return g_sparse_heads;
}
static int g_static_weights = 0;   // option "static_weights" (see forward_impl)
static long g_static_gen = 0;      // bumped by every set_option("static_weights", v)

struct frcnn_model {
  frcnn_model_desc d;
  std::vector<Conv> convs;     // backbone convs in order
  std::vector<Block> blocks;
  std::vector<Head> heads;
  std::vector<ClsLayer> cls;
  long pnet_params = 0, total_params = 0;
  long bbox_w_off = 0, bbox_b_off = 0, clsw_off = 0, clsb_off = 0;
  int H = 0, W = 0;            // current image size
  int training = 0;
  DevBuf delta_last;           // delta_outputs[nheads+1]
  DevBuf zero_arena;           // delta_outputs[1..n+1] followed by the pooled-map gradients: zeroed by ONE memset each
  size_t delta_bytes = 0, gpool_bytes = 0;
  PackTables packs;            // the device job tables of the weight packs and their named parts (pack_tables.h)
  // Two-plane fp16 form of the split launches (option x3_f16): every tensor such a launch reads is scaled by a power of two that
  // puts its largest magnitude just below the end of the fp16 range, so the magnitudes travel with the tensors -- one record
  // (amax.h: a maximum per block of the launch that wrote the tensor) per convolution output, output gradient, weight tensor and
  // pooled map; amax_ws[c.am] = the weight tensor's largest magnitude as a scalar (published by the pack).
  DevBuf amax, amax_ws;        // the records; the weight scalars
  int n_amax = 0;
  float* rec(int id) const { return (float*)amax.p + (size_t)id * AMAX_REC; }
  // am_live[id]: record id was handed to the launch that writes it in the last pass (forward pass: outputs, pooled maps, weights;
  // backward pass: output gradients) -- what frcnn_model_debug_buffer's record kinds may show.  rec_w: rec for a producer.
  std::vector<unsigned char> am_live;
  float* rec_w(int id) { am_live[id] = 1; return rec(id); }
  // the weight records a tensor_absmax_multi launch of the forward pass writes: every owner's, or the backbone's only
  void weights_live(bool heads_too) {
    for (auto& t : packs.tensors) if (t.has_record() && (heads_too || !t.head())) am_live[t.am + 2] = 1;
  }
  bool f16_packed = false;     // the current packs are in the fp16 form
  long eval_packs_gen = -1;    // option static_weights: generation (g_static_gen) the evaluate-mode packs were made in, -1 = none
  const float* eval_packs_w = nullptr;
  bool head_packs_fresh = false;   // head input-gradient packs match the weights of the last forward
  unsigned fresh_mask = 0;         // bit g: group g's training packs were renewed by frcnn_pnet_refresh_packs since the last forward
  const float* fresh_w = nullptr;  // ... from this weight vector
  bool fresh_f16 = false;          // ... in this form
  // per-step tables of the compact blocks (see Block::dc_on): a ring of page-locked host slots and device slots, one
  // asynchronous copy per step: [PackXJob table of the step][kept-channel tables of the blocks]
  static const int DC_RING = 4;
  PinBuf dc_pin; DevBuf dc_dev; size_t dc_slot_bytes = 0, dc_idx_off = 0; unsigned dc_step = 0;
  Event dc_ev[DC_RING];                       // slot s's copy to the device has run (a host that queues more than DC_RING passes ahead waits here)
  DevBuf dbg_expand;                          // frcnn_model_debug_buffer: a compact tensor laid out dense
  std::vector<Event> block_rd_ev;   // block b's weights and packs have been read for the last time (caller's stream, frcnn_pnet_backward)
  hipStream_t side = nullptr;      // accGradParameters stream (runs beside the updateGradInput chain)
  hipStream_t cw = nullptr;        // the classification net's weight gradients / bias sums (beside its input-gradient chain)
  Event cw_done;                   // last work queued on `cw`
  bool cw_pending = false;         // work on `cw` that no stream has been made to wait for yet
  std::vector<Event> cw_ev;        // one fork point per layer + one for the two heads
  std::vector<Event> fork_ev;      // fork points of the side stream and the anchor nets' streams (fork_to)
  Event join_ev;                   // join point of the side stream (join_side_now)
  bool update_armed = false;       // a host has asked for the update stream (frcnn_model_update_stream): the passes record the
                                   // events its waits need (bwd_ev, block_rd_ev) -- each costs the caller's stream a marker packet
  Event bwd_ev;                    // the backbone's backward pass has begun on the caller's stream (anchor nets joined)
  Event upd_ev, upd_join_ev;       // fork / join points of the update stream (frcnn_model_update_*)
  bool head_x3_fresh = true;       // the anchor nets' split-operand packs and weight magnitudes match the last forward pass's weights
  bool heads_deferred = false;     // training pass: the anchor nets' forward part has not been launched yet (frcnn_pnet_forward_async_heads
                                   // leaves it to the call that knows the sampled positions: heads.hip)
  bool heads_sparse_fwd = false;   // ... and was then computed at the sampled positions only
  const float* last_w = nullptr;   // weight vector of the last forward pass
  Event heads_gin_ev;              // sparse path: the anchor nets' contributions to the pooled maps' gradients have been added (side stream)
  bool heads_gin = false;
  bool heads_begun = false;        // anchor-net backward already running on the side stream
  bool heads_joined = false;       // ... and the caller's stream already waits for it
  bool side_busy = false;          // work was forked to the side stream and not joined yet
  Event loss_ev;                   // anchor losses of frcnn_pnet_anchor_loss_begin are final (side stream)
  Event chain_ev;                  // ... and the pooled-map gradient buffers are zeroed: the anchor nets' backward may start
  std::vector<Event> block_ev;     // block b's parameter gradients are final (recorded by frcnn_pnet_backward)
  bool block_ev_valid = false;
  bool loss_pending = false;
  DevBuf wg_ws;                // split-K slab workspace of the weight-gradient kernels
  DevBuf wg_ws_first;          // ... of the first layer's, which runs on the caller's stream beside the side stream's last launches
  DevBuf img;                  // copy of the input image (needed by the first conv's accGradParameters)
  // staged training (frcnn_model_set_trainable): backbone blocks 0..frozen_blocks-1, the anchor nets (train_heads = 0) and the
  // classification net (train_cnet = 0) are held fixed -- the training entry points queue no launch that only serves them
  int frozen_blocks = 0;
  int train_heads = 1, train_cnet = 1;
  // cnet state
  int R = 0, D = 0;
  const float* cnet_x = nullptr;
  DevBuf feat_g, logits, lsm, glog, gtmp;
  // the per-class box head (desc.box_per_class; box_head.hip): the class each row of the last forward pass used, and the class
  // source frcnn_cnet_box_classes set for the NEXT forward pass (0: none -- the first maximum of the pass's own log-probabilities)
  DevBuf box_sel;
  const void* box_classes = nullptr;
  int box_kind = 0, box_n = 0;
  std::vector<std::array<long long, 4>> table;
};

// one launch per job kind from a named part of its table (an empty span queues nothing)
static int run_packs(const frcnn_model* m, const float* w, const Span& sp, hipStream_t s) { return conv_pack_weights_multi(w, m->packs.pack.at(sp), sp.n, sp.grid, s); }
static int run_amax(const frcnn_model* m, const float* w, const Span& sp, hipStream_t s) { return tensor_absmax_multi(w, m->packs.amax.at(sp), sp.n, sp.grid, s); }
static int run_x3_packs(const frcnn_model* m, const float* w, const Span& sp, hipStream_t s) { return conv_x3_pack_multi(w, m->packs.x3.at(sp), sp.n, sp.grid, s); }

static int pool_out(int n) { return (n - 2 + 1) / 2 + 1; }
static int refresh_group(frcnn_model* m, const float* w, int group, hipStream_t s);

static void build_layout(frcnn_model* m) {
  const frcnn_model_desc& d = m->d;
  long off = 0;
  int cin = 3;
  for (int b = 0; b < d.nblocks; ++b) {
    Block blk;
    blk.first_conv = (int)m->convs.size();
    blk.nconv = d.conv_steps[b];
    blk.has_drop = d.dropout[b] > 0.f;  // model_utilities.lua:10
    blk.p_drop = d.dropout[b];
    for (int s = 0; s < d.conv_steps[b]; ++s) {
      Conv c;
      c.Cin = cin; c.Cout = d.filters[b]; c.k = d.ksize[b]; c.pad = d.pad[b];
      c.block = b; c.step = s;
      long wsz = (long)c.Cout * c.Cin * c.k * c.k;
      c.w_off = off; c.b_off = off + wsz; c.a_off = off + wsz + c.Cout;
      m->table.push_back({c.w_off, wsz, 0, (long long)c.k * c.k * c.Cout});
      m->table.push_back({c.b_off, c.Cout, 1, 0});
      m->table.push_back({c.a_off, 1, 2, 0});
      off += wsz + c.Cout + 1;
      cin = c.Cout;
      m->convs.push_back(std::move(c));
    }
    m->blocks.push_back(std::move(blk));
  }
  for (int h = 0; h < d.nheads; ++h) {
    Head hd;
    hd.input = d.head_input[h] - 1;
    Conv& a = hd.c3;
    a.Cin = d.filters[hd.input]; a.Cout = d.head_n[h]; a.k = d.head_k[h]; a.pad = 0;
    a.block = -1; a.step = 0;
    long wsz = (long)a.Cout * a.Cin * a.k * a.k;
    a.w_off = off; a.b_off = off + wsz; a.a_off = off + wsz + a.Cout;
    m->table.push_back({a.w_off, wsz, 0, (long long)a.k * a.k * a.Cout});
    m->table.push_back({a.b_off, a.Cout, 1, 0});
    m->table.push_back({a.a_off, 1, 2, 0});
    off += wsz + a.Cout + 1;
    Conv& c = hd.c1;
    c.Cin = a.Cout; c.Cout = HEAD_OUT; c.k = 1; c.pad = 0; c.block = -1; c.step = 1;
    long w1 = (long)HEAD_OUT * c.Cin;
    c.w_off = off; c.b_off = off + w1; c.a_off = -1;
    m->table.push_back({c.w_off, w1, 0, (long long)HEAD_OUT});
    m->table.push_back({c.b_off, HEAD_OUT, 1, 0});
    off += w1 + HEAD_OUT;
    m->heads.push_back(std::move(hd));
  }
  m->pnet_params = off;
  int in = d.kh * d.kw * d.filters[d.nblocks - 1];  // model_utilities.lua:127
  m->D = in;
  for (int l = 0; l < d.ncls; ++l) {
    ClsLayer L;
    L.in = in; L.n = d.cls_n[l]; L.bn = d.cls_bn[l] != 0; L.p_drop = d.cls_dropout[l];
    L.w_off = off; L.b_off = off + (long)in * L.n;
    m->table.push_back({L.w_off, (long long)in * L.n, 3, in});
    m->table.push_back({L.b_off, L.n, 4, in});
    off += (long)in * L.n + L.n;
    L.bnw_off = L.bnb_off = -1;
    if (L.bn) {
      L.bnw_off = off; L.bnb_off = off + L.n;
      m->table.push_back({L.bnw_off, L.n, 5, 0});
      m->table.push_back({L.bnb_off, L.n, 6, 0});
      off += 2L * L.n;
    }
    L.a_off = off;
    m->table.push_back({L.a_off, 1, 2, 0});
    off += 1;
    in = L.n;
    m->cls.push_back(std::move(L));
  }
  const int brows = d.box_per_class ? 4 * d.class_count : 4;   // per class: row 4 (c - 1) + j = coordinate j of foreground class c
  m->bbox_w_off = off; m->bbox_b_off = off + (long)in * brows;
  m->table.push_back({m->bbox_w_off, (long long)in * brows, 3, in});
  m->table.push_back({m->bbox_b_off, brows, 4, in});
  off += (long)in * brows + brows;
  int nc = d.class_count + 1;
  m->clsw_off = off; m->clsb_off = off + (long)in * nc;
  m->table.push_back({m->clsw_off, (long long)in * nc, 3, in});
  m->table.push_back({m->clsb_off, nc, 4, in});
  off += (long)in * nc + nc;
  m->total_params = off;
  // the events by index (none is made before its first record: see Event)
  m->block_ev.resize(m->blocks.size());
  m->block_rd_ev.resize(m->blocks.size());
  m->cw_ev.resize(m->cls.size() + 1);
  // (fork_ev: one per backbone convolution in frcnn_pnet_backward, nblocks + 1 for the anchor nets' backward, 16 + i for anchor net i)
  m->fork_ev.resize(std::max({m->convs.size(), m->blocks.size() + 2, 16 + m->heads.size()}));
}

static int ensure_conv(Conv& c, int H, int W, bool need_dgrad) {
  c.H = H; c.W = W;
  c.Ho = H + 2 * c.pad - c.k + 1; c.Wo = W + 2 * c.pad - c.k + 1;
  FR_CHECK(c.Ho > 0 && c.Wo > 0, "image too small: a %dx%d map reaches a %dx%d convolution", H, W, c.k, c.k);
  size_t n = (size_t)c.Cout * c.Ho * c.Wo * 4;
  FR_TRY(c.x.ensure(n));
  FR_TRY(c.gx.ensure(n));
  // packed weights: the padding (channels beyond C, columns beyond M) is zeroed once here and never written again
  if (c.wf.bytes < conv_pack_floats(c.Cin, c.Cout, c.k) * 4) {
    FR_TRY(c.wf.ensure(conv_pack_floats(c.Cin, c.Cout, c.k) * 4));
    FR_HIP(hipMemset(c.wf.p, 0, c.wf.bytes));
  }
  if (need_dgrad && c.wd.bytes < conv_pack_floats(c.Cout, c.Cin, c.k) * 4) {
    FR_TRY(c.wd.ensure(conv_pack_floats(c.Cout, c.Cin, c.k) * 4));
    FR_HIP(hipMemset(c.wd.p, 0, c.wd.bytes));
  }
  // Launches whose shape fits take the split-bf16 operand form (convx.hip): fp32 results at 6/16 of the matrix-pipe time.  The 3x3
  // layers since round 2; the 5x5 / 7x7 anchor nets since round 5: rounds 2 and 3 had measured them slower in that form (8x10-pixel
  // tiles under the 204-position patch limit; then 8x16 tiles but a stage loop that needed three resident blocks to hide its LDS
  // round trips: 3.14 against 3.11 ms/step).  With the stage pipelined inside the wave (convx.hip) two blocks per CU suffice: the 7x7
  // net 118.8 -> 63.8 us alone, the 5x5 net 67.4 -> 56.8, the step 2.918 -> 2.834 ms.
  c.x_f = (c.k == 3 || c.block < 0) && conv_x3_eligible(c.Cin, c.Cout, c.k);
  c.x_d = c.block >= 0 && need_dgrad && conv_x3_eligible(c.Cout, c.Cin, c.k);
  if (c.x_f) FR_TRY(c.wx.ensure(conv_x3_pack_bytes(c.Cin, c.Cout, c.k)));
  if (c.x_d) FR_TRY(c.wxd.ensure(conv_x3_pack_bytes(c.Cout, c.Cin, c.k)));
  return FRCNN_OK;
}

// a convolution's entry in the enumeration the pack-job tables are built from (pack_tables.h)
static PackTensor pack_tensor(const Conv& c, PackTensor::Kind kind, int group, int conv) {
  PackTensor t;
  t.kind = kind; t.group = group; t.conv = conv; t.first = c.block == 0 && c.step == 0;
  t.x_f = c.x_f; t.x_d = c.x_d; t.am = c.am;
  t.w_off = c.w_off; t.Cout = c.Cout; t.Cin = c.Cin; t.k = c.k; t.H = c.H; t.W = c.W; t.Ho = c.Ho; t.Wo = c.Wo;
  t.wf = c.wf.f(); t.wd = c.wd.f(); t.wx = c.wx.p; t.wxd = c.wxd.p;
  return t;
}

static int ensure_shapes(frcnn_model* m, int H, int W) {
  int h = H, w = W;
  for (size_t b = 0; b < m->blocks.size(); ++b) {
    Block& blk = m->blocks[b];
    for (int s = 0; s < blk.nconv; ++s) {
      Conv& c = m->convs[blk.first_conv + s];
      FR_TRY(ensure_conv(c, h, w, !(b == 0 && s == 0)));
      h = c.Ho; w = c.Wo;
    }
    FR_CHECK(h >= 2 && w >= 2, "image too small for block %zu pooling", b + 1);
    blk.Hp = pool_out(h); blk.Wp = pool_out(w);
    int C = m->d.filters[b];
    FR_TRY(blk.pooled.ensure((size_t)C * blk.Hp * blk.Wp * 4));
    FR_TRY(blk.pidx.ensure((size_t)C * blk.Hp * blk.Wp));
    if (blk.has_drop) FR_TRY(blk.scale.ensure((size_t)C * 4));
    h = blk.Hp; w = blk.Wp;
  }
  for (auto& hd : m->heads) {
    const Block& in = m->blocks[hd.input];
    FR_TRY(ensure_conv(hd.c3, in.Hp, in.Wp, true));
    FR_TRY(ensure_conv(hd.c1, hd.c3.Ho, hd.c3.Wo, true));
  }
  const Block& last = m->blocks.back();
  {  // one arena: [deltas of the heads | delta of the last map | gpooled of every block]
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    size_t db = 0, gb = 0;
    for (auto& hd : m->heads) db += al((size_t)HEAD_OUT * hd.c1.Ho * hd.c1.Wo * 4);
    db += al((size_t)m->d.filters[m->d.nblocks - 1] * last.Hp * last.Wp * 4);
    for (size_t b = 0; b < m->blocks.size(); ++b) gb += al((size_t)m->d.filters[b] * m->blocks[b].Hp * m->blocks[b].Wp * 4);
    m->zero_arena.release();
    FR_TRY(m->zero_arena.ensure(db + gb));
    char* q = (char*)m->zero_arena.p;
    for (auto& hd : m->heads) { size_t n = (size_t)HEAD_OUT * hd.c1.Ho * hd.c1.Wo * 4; hd.delta.view(q, n); q += al(n); }
    { size_t n = (size_t)m->d.filters[m->d.nblocks - 1] * last.Hp * last.Wp * 4; m->delta_last.view(q, n); q += al(n); }
    for (size_t b = 0; b < m->blocks.size(); ++b) {
      size_t n = (size_t)m->d.filters[b] * m->blocks[b].Hp * m->blocks[b].Wp * 4;
      m->blocks[b].gpooled.view(q, n); q += al(n);
    }
    m->delta_bytes = db; m->gpool_bytes = gb;
  }
  size_t wsb = 0;
  for (auto& c : m->convs) wsb = std::max(wsb, conv_wgrad_workspace_bytes(c.Cin, c.H, c.W, c.Cout, c.k, c.pad));
  for (auto& hd : m->heads) {
    wsb = std::max(wsb, conv_wgrad_workspace_bytes(hd.c3.Cin, hd.c3.H, hd.c3.W, hd.c3.Cout, hd.c3.k, 0));
    wsb = std::max(wsb, conv_wgrad_workspace_bytes(hd.c1.Cin, hd.c1.H, hd.c1.W, hd.c1.Cout, 1, 0));
  }
  FR_TRY(m->wg_ws.ensure(wsb));
  { const Conv& c0 = m->convs[0]; FR_TRY(m->wg_ws_first.ensure(conv_wgrad_workspace_bytes(c0.Cin, c0.H, c0.W, c0.Cout, c0.k, c0.pad))); }
  {  // magnitude records of the two-plane fp16 form (see frcnn_model::amax)
    int n = 0;
    for (auto& c : m->convs) { c.am = n; n += 3; }
    for (auto& hd : m->heads) { hd.c3.am = n; n += 3; }
    for (auto& b : m->blocks) b.am = n++;
    m->n_amax = n;
    m->am_live.assign((size_t)n, 0);
    FR_TRY(m->amax.ensure((size_t)n * AMAX_REC * 4));
    FR_TRY(m->amax_ws.ensure((size_t)n * 4));
  }
  {  // the pack-job tables (buffers may have been re-allocated above)
    const int nb = (int)m->blocks.size();
    std::vector<PackTensor> ts;
    for (size_t i = 0; i < m->convs.size(); ++i) ts.push_back(pack_tensor(m->convs[i], PackTensor::BACKBONE, m->convs[i].block, (int)i));
    for (auto& hd : m->heads) {
      ts.push_back(pack_tensor(hd.c3, PackTensor::HEAD_C3, nb, -1));
      ts.push_back(pack_tensor(hd.c1, PackTensor::HEAD_C1, nb, -1));
    }
    FR_TRY(m->packs.build(std::move(ts), nb, m->amax.f(), m->amax_ws.f()));
    FR_TRY(m->packs.upload());
  }
  {  // ring of per-step tables: [PackXJob x jobs][int x channels of every block], see frcnn_model::dc_pin
    size_t chans = 0;
    for (size_t b = 0; b < m->blocks.size(); ++b) chans += (size_t)m->d.filters[b];
    m->dc_idx_off = (m->packs.x3_train[0].n * sizeof(PackXJob) + 255) / 256 * 256;
    const size_t slot = (m->dc_idx_off + chans * 4 + 255) / 256 * 256;
    if (slot != m->dc_slot_bytes) {   // a new ring: no slot has a copy in flight, the first pass takes slot 0
      for (auto& e : m->dc_ev) e.reset();
      m->dc_step = 0;
      FR_TRY(m->dc_pin.alloc(slot * frcnn_model::DC_RING));
      m->dc_dev.release();
      FR_TRY(m->dc_dev.ensure(slot * frcnn_model::DC_RING));
      m->dc_slot_bytes = slot;
    }
    for (size_t b = 0; b < m->blocks.size(); ++b)
      if (m->blocks[b].has_drop) FR_TRY(m->blocks[b].dc_bias.ensure((size_t)m->d.filters[b] * 4));
  }
  m->H = H; m->W = W;
  m->eval_packs_gen = -1;   // (pack buffers and job tables were rebuilt)
  m->fresh_mask = 0;
  return FRCNN_OK;
}

extern "C" {

int frcnn_model_create(const frcnn_model_desc* desc, frcnn_model** out) {
  FR_CHECK(desc && out, "frcnn_model_create: null argument");
  FR_CHECK(desc->nblocks >= 1 && desc->nblocks <= 8 && desc->nheads >= 0 && desc->nheads <= 8 &&
               desc->ncls >= 0 && desc->ncls <= 8,
           "frcnn_model_create: bad layer counts");
  for (int b = 0; b < desc->nblocks; ++b) {
    FR_CHECK(desc->ksize[b] == 1 || desc->ksize[b] == 3 || desc->ksize[b] == 5 || desc->ksize[b] == 7,
             "block %d: kernel size %d unsupported (1,3,5,7)", b + 1, desc->ksize[b]);
    FR_CHECK(desc->conv_steps[b] >= 1, "block %d: conv_steps must be >= 1", b + 1);
  }
  for (int h = 0; h < desc->nheads; ++h) {
    FR_CHECK(desc->head_input[h] >= 1 && desc->head_input[h] <= desc->nblocks, "anchor net %d: bad input", h + 1);
    FR_CHECK(desc->head_k[h] == 1 || desc->head_k[h] == 3 || desc->head_k[h] == 5 || desc->head_k[h] == 7,
             "anchor net %d: kernel size %d unsupported", h + 1, desc->head_k[h]);
  }
  FR_CHECK(!desc->box_per_class || desc->class_count >= 1, "frcnn_model_create: box_per_class with %d classes", desc->class_count);
  frcnn_model* m = new frcnn_model();
  m->d = *desc;
  build_layout(m);
  *out = m;
  return FRCNN_OK;
}

int frcnn_model_destroy(frcnn_model* m) {
  if (!m) return FRCNN_OK;
  delete m;   // (every buffer and event is given back by its field's type)
  return FRCNN_OK;
}

int frcnn_model_param_count(const frcnn_model* m, long long* total, long long* pnet) {
  if (total) *total = m->total_params;
  if (pnet) *pnet = m->pnet_params;
  return FRCNN_OK;
}

int frcnn_model_param_table(const frcnn_model* m, long long* table, int cap, int* n) {
  *n = (int)m->table.size();
  for (int i = 0; i < *n && i < cap; ++i)
    for (int j = 0; j < 4; ++j) table[4 * i + j] = m->table[i][j];
  return FRCNN_OK;
}

int frcnn_model_set_trainable(frcnn_model* m, int frozen_blocks, int heads, int cnet) {
  const int nb = (int)m->blocks.size();
  FR_CHECK(frozen_blocks >= 0 && frozen_blocks <= nb, "model_set_trainable: frozen_blocks %d outside 0..%d", frozen_blocks, nb);
  // (with a stage on, something is trainable: its own net)
  FR_CHECK(heads || cnet, "model_set_trainable: both stages are off (no loss is back-propagated, no parameter to train)");
  m->frozen_blocks = frozen_blocks;
  m->train_heads = heads != 0;
  m->train_cnet = cnet != 0;
  return FRCNN_OK;
}

int frcnn_model_get_trainable(const frcnn_model* m, int* frozen_blocks, int* heads, int* cnet) {
  if (frozen_blocks) *frozen_blocks = m->frozen_blocks;
  if (heads) *heads = m->train_heads;
  if (cnet) *cnet = m->train_cnet;
  return FRCNN_OK;
}

int frcnn_model_localizer_layers(const frcnn_model* m, int output_index, int* layers, int cap, int* n_out) {
  const frcnn_model_desc& d = m->d;
  FR_CHECK(output_index >= 1 && output_index <= d.nheads + 1, "localizer: output index %d out of range", output_index);
  int nb = output_index <= d.nheads ? d.head_input[output_index - 1] : d.nblocks;
  int n = 0;
  auto push = [&](int kW, int kH, int dW, int dH, int pW, int pH) {
    if (n < cap) { int* l = layers + 6 * n; l[0] = kW; l[1] = kH; l[2] = dW; l[3] = dH; l[4] = pW; l[5] = pH; }
    ++n;
  };
  for (int b = 0; b < nb; ++b) {
    for (int s = 0; s < d.conv_steps[b]; ++s) push(d.ksize[b], d.ksize[b], 1, 1, d.pad[b], d.pad[b]);
    push(2, 2, 2, 2, 0, 0);
  }
  if (output_index <= d.nheads) {
    int k = d.head_k[output_index - 1];
    push(k, k, 1, 1, 0, 0);
    push(1, 1, 1, 1, 0, 0);
  }
  *n_out = n;
  return FRCNN_OK;
}

// ------------------------------------------------------------------------------------ pnet
static int g_side_stream = -1;   // -1: not decided yet (environment FRCNN_SIDE_STREAM, default on)
static bool side_enabled() {
  if (g_side_stream < 0) g_side_stream = env_flag("FRCNN_SIDE_STREAM", true);
  return g_side_stream != 0;
}

// The classification net's weight-gradient products and bias sums are needed by nobody before the optimiser (or the exchange of
// the cnet slice): with the option on (default) frcnn_cnet_backward queues them on a stream of their own, beside the
// input-gradient chain that the ROI-pooling backward and the backbone wait for, and returns with that stream still busy --
// frcnn_pnet_backward, the next frcnn_cnet_forward and frcnn_cnet_backward_join make the caller's stream wait for it.
static int g_cnet_wgrad_async = env_flag("FRCNN_CNET_WGRAD_ASYNC", true);

// stream `to` waits for everything enqueued on `from` so far (event ev is re-recorded: its previous waiters are queued already).
// The one place that pairs a record with a wait.
static int chain(hipStream_t from, hipStream_t to, Event& ev) {
  if (from == to) return FRCNN_OK;
  FR_TRY(ev.record(from));
  return ev.wait(to);
}

static int cw_join(frcnn_model* m, hipStream_t s) {
  if (m->cw_pending) {
    FR_TRY(m->cw_done.wait(s));
    m->cw_pending = false;
  }
  return FRCNN_OK;
}

int frcnn_cnet_backward_join(frcnn_model* m, void* stream) {
  FR_CHECK(m != nullptr, "cnet_backward_join: null model");
  return cw_join(m, S(stream));
}

// The update stream: a library-owned stream on which the host queues the optimiser's update of a slice of the flat vectors (and
// the renewal of the packs made from it) while the caller's stream is still busy with the rest of the backward pass.  It is the
// stream the classification net's weight gradients run on -- idle from the end of that stage to the end of the step -- so a
// slice update queued on it is ordered behind those gradients by itself.
static int ensure_update_stream(frcnn_model* m) { return m->cw ? FRCNN_OK : pool_stream(1, &m->cw); }
int frcnn_model_update_stream(frcnn_model* m, void** stream) {
  FR_CHECK(m && stream, "model_update_stream: null argument");
  FR_TRY(ensure_update_stream(m));
  m->update_armed = true;
  *stream = (void*)m->cw;
  return FRCNN_OK;
}
// the update stream waits for everything queued on `stream` so far (the last readers of the weights about to be updated)
int frcnn_model_update_fork(frcnn_model* m, void* stream) {
  FR_CHECK(m != nullptr, "model_update_fork: null model");
  FR_TRY(ensure_update_stream(m));
  return chain(S(stream), m->cw, m->upd_ev);
}
// `stream` waits for everything queued on the update stream so far (before the next pass reads the weights and the packs)
int frcnn_model_update_join(frcnn_model* m, void* stream) {
  FR_CHECK(m != nullptr, "model_update_join: null model");
  FR_TRY(ensure_update_stream(m));
  return chain(m->cw, S(stream), m->upd_join_ev);
}

int frcnn_get_option(const char* name, int* value) {
  FR_CHECK(name != nullptr && value != nullptr, "get_option: null argument");
  if (strcmp(name, "side_stream") == 0) { *value = side_enabled() ? 1 : 0; return FRCNN_OK; }
  if (strcmp(name, "gemm_x_roles") == 0) { *value = get_gemm_x_roles(); return FRCNN_OK; }
  if (strcmp(name, "deterministic") == 0) { *value = deterministic() ? 1 : 0; return FRCNN_OK; }
  if (strcmp(name, "static_weights") == 0) { *value = g_static_weights; return FRCNN_OK; }
  if (strcmp(name, "drop_compact") == 0) { *value = drop_compact_on(); return FRCNN_OK; }
  if (strcmp(name, "sparse_heads") == 0) { *value = sparse_heads_on(); return FRCNN_OK; }
  if (strcmp(name, "winograd") == 0) { *value = 0; return FRCNN_OK; }   // removed in round 3; kept as a name that reads 0
  if (strcmp(name, "cnet_wgrad_async") == 0) { *value = g_cnet_wgrad_async; return FRCNN_OK; }
  if (strcmp(name, "split_bf16") == 0) { *value = get_split_bf16(); return FRCNN_OK; }
  if (strcmp(name, "x3_f16") == 0) { *value = get_x3_f16(); return FRCNN_OK; }
  FR_CHECK(false, "get_option: unknown option '%s'", name);
  return FRCNN_OK;
}

int frcnn_set_option(const char* name, int value) {
  FR_CHECK(name != nullptr, "set_option: null name");
  if (strcmp(name, "side_stream") == 0) { g_side_stream = value ? 1 : 0; return FRCNN_OK; }
  if (strcmp(name, "deterministic") == 0) { set_deterministic(value != 0); return FRCNN_OK; }
  if (strcmp(name, "static_weights") == 0) { g_static_weights = value != 0; ++g_static_gen; return FRCNN_OK; }
  if (strcmp(name, "drop_compact") == 0) { g_drop_compact = value != 0; return FRCNN_OK; }
  if (strcmp(name, "sparse_heads") == 0) { g_sparse_heads = value != 0; return FRCNN_OK; }
  if (strcmp(name, "gemm_x_roles") == 0) { set_gemm_x_roles(value); return FRCNN_OK; }   // takes effect at the next cnet pass
  if (strcmp(name, "split_bf16") == 0) { set_split_bf16(value); return FRCNN_OK; }   // takes effect for models shaped afterwards
  if (strcmp(name, "x3_f16") == 0) { set_x3_f16(value); return FRCNN_OK; }           // takes effect with the next forward pass
  if (strcmp(name, "winograd") == 0) return FRCNN_OK;   // deprecated no-op: the Winograd kernels were removed in round 3
  if (strcmp(name, "cnet_wgrad_async") == 0) { g_cnet_wgrad_async = value ? 1 : 0; return FRCNN_OK; }
  FR_CHECK(false, "set_option: unknown option '%s'", name);
  return FRCNN_OK;
}

static int ensure_side(frcnn_model* m) { return m->side ? FRCNN_OK : pool_stream(0, &m->side); }

// The anchor nets' own streams, made when the DENSE path first needs them (round 6): a stream that exists takes a share of a
// hardware queue whether it is used or not, and the sparse training path (heads.hip) runs every anchor net on the side stream.
static int ensure_head_streams(frcnn_model* m) {
  // FRCNN_HEAD_STREAMS=1: one stream per anchor net (the four nets are independent of each other: forward a k x k and
  // a 1 x 1 convolution on a pooled map; backward on the sampled anchors ~17 small launches each), so that their chains
  // run beside each other instead of one after the other.  Measured on the training step: the anchor nets' backward
  // chains shrink from 670 to 310 us, but the classification net's chain on the caller's stream, which runs beside them,
  // slows down by as much: 223.6 against 225.4 images/s (round 2).  Round 4: the two chains of the middle phase -- the
  // anchor nets' and the classification net's -- are about equally long, so shortening ONE of them changes nothing; with
  // the classification net's weight gradients off its chain as well (g_cnet_wgrad_async) the step goes from 3.11 to
  // 3.02 ms, with either change alone it stays at 3.11.  On by default since then.
  static const bool head_streams = env_flag("FRCNN_HEAD_STREAMS", true);
  size_t hi = 0;
  for (auto& h : m->heads) {
    // (five workspace slots for streams of their own, head_slot(): a sixth anchor net shares the side stream and its slot)
    if (head_streams && hi < 5 && !h.stream) FR_TRY(pool_stream(2 + (int)hi, &h.stream));
    ++hi;
  }
  return FRCNN_OK;
}

static hipStream_t head_stream(frcnn_model* m, size_t i) { return m->heads[i].stream ? m->heads[i].stream : m->side; }
// split-K workspace slot of anchor net i: 2..6 (slot 7 belongs to the classification net's weight-gradient stream, 0 / 1 to the
// caller's and the side stream); build_layout gives streams of their own to at most five anchor nets
static int head_slot(frcnn_model* m, size_t i) { return m->heads[i].stream ? 2 + (int)(i % 5) : 1; }

// stream s waits for everything queued on the anchor nets' own streams so far
static int join_heads(frcnn_model* m, hipStream_t s) {
  for (auto& h : m->heads)
    if (h.stream) FR_TRY(chain(h.stream, s, h.done));
  return FRCNN_OK;
}
// ... for everything queued on the side stream so far
static int join_side_now(frcnn_model* m, hipStream_t s) { return chain(m->side, s, m->join_ev); }
// the caller's stream waits for whatever was forked off it and not joined yet: the anchor nets' streams and the side stream
static int join_side(frcnn_model* m, hipStream_t s) {
  if (!m->side || !m->side_busy) return FRCNN_OK;
  FR_TRY(join_heads(m, s));
  FR_TRY(join_side_now(m, s));
  m->side_busy = false;
  return FRCNN_OK;
}

// stream `to` (the side stream or an anchor net's own) waits for everything enqueued on `s` so far
static int fork_to(frcnn_model* m, hipStream_t s, hipStream_t to, size_t idx) {
  FR_TRY(ensure_side(m));
  FR_TRY(chain(s, to, m->fork_ev[idx]));
  m->side_busy = true;
  return FRCNN_OK;
}
static int fork_side(frcnn_model* m, hipStream_t s, size_t idx) {
  FR_TRY(ensure_side(m));
  return fork_to(m, s, m->side, idx);
}

// one anchor net: k x k conv -> PReLU (fused into the 1x1 loader) -> 1x1 conv (models/model_utilities.lua:31-34)
static int head_forward(frcnn_model* m, Head& h, const float* w, hipStream_t s, int ws_slot) {
  const Block& in = m->blocks[h.input];
  if (h.c3.x_f)
    FR_TRY(conv_x3(in.pooled.f(), h.c3.Cin, h.c3.H, h.c3.W, nullptr, nullptr, h.c3.wx.p, w + h.c3.b_off, h.c3.Cout, h.c3.k, 0,
                   h.c3.x.f(), OUT_STORE, 0, s, ws_slot, nullptr, m->f16_packed ? m->rec(in.am) : nullptr,
                   m->f16_packed ? m->amax_ws.f() + h.c3.am : nullptr));
  else
    FR_TRY(conv_igemm(in.pooled.f(), h.c3.Cin, h.c3.H, h.c3.W, nullptr, nullptr, h.c3.wf.f(), w + h.c3.b_off,
                      h.c3.Cout, h.c3.k, 0, h.c3.x.f(), OUT_STORE, 0, s, ws_slot));
  FR_TRY(conv_igemm(h.c3.x.f(), h.c1.Cin, h.c1.H, h.c1.W, w + h.c3.a_off, nullptr, h.c1.wf.f(), w + h.c1.b_off,
                    HEAD_OUT, 1, 0, h.c1.x.f(), OUT_STORE, 0, s, ws_slot));
  return FRCNN_OK;
}

// ---- compact blocks (Block::dc_on) --------------------------------------------------------------------------------------
static bool any_compact(const frcnn_model* m) {
  for (auto& b : m->blocks) if (b.dc_on) return true;
  return false;
}
static bool fuse_act_on() { return !deterministic() && env_flag("FRCNN_FUSE_ACT", true); }   // (read per call: the tests switch it)

// Decides, block by block, whether this training pass runs compact, from the keep vectors -- drawn here with the very hash the
// device kernel uses (common.h frcnn_keep_mask: the vectors on the device and on the host are the same), or read back from the
// caller's explicit masks (a synchronous copy: parity runs only) -- and fills the step's slot of the table ring with the kept
// channels.  The job table follows in pack_compact.
static int plan_compact(frcnn_model* m, int training, const float* const* drop_masks, unsigned long long seed) {
  for (auto& b : m->blocks) { b.dc_on = false; b.dc_idx = nullptr; }
  if (!training || !drop_compact_on() || !fuse_act_on() || !m->dc_pin.p) return FRCNN_OK;
  const unsigned slot = m->dc_step % frcnn_model::DC_RING;
  FR_TRY(m->dc_ev[slot].sync());   // (the slot's previous copy, DC_RING passes ago: long done unless the host never looks back)
  int* idx_host = (int*)(m->dc_pin.p + (size_t)slot * m->dc_slot_bytes + m->dc_idx_off);
  const int* idx_dev = (const int*)((char*)m->dc_dev.p + (size_t)slot * m->dc_slot_bytes + m->dc_idx_off);
  size_t at = 0;
  std::vector<float> keep;
  for (size_t b = 0; b < m->blocks.size(); ++b) {
    Block& blk = m->blocks[b];
    const int C = m->d.filters[b];
    const size_t my = at;
    at += (size_t)C;
    if (!blk.has_drop || blk.nconv < 2) continue;
    Conv &c0 = m->convs[blk.first_conv], &c1 = m->convs[blk.first_conv + 1];
    if (!(c0.k == 3 && c1.k == 3 && c0.x_f && c1.x_f && c1.x_d && (b == 0 || c0.x_d))) continue;
    keep.resize(C);
    if (drop_masks && drop_masks[b]) {
      FR_HIP(hipMemcpy(keep.data(), drop_masks[b], (size_t)C * 4, hipMemcpyDeviceToHost));
    } else {
      for (int i = 0; i < C; ++i) keep[i] = frcnn_keep_mask(seed * 131 + b, (unsigned long long)i, blk.p_drop);
    }
    int nk = 0;
    bool binary = true;
    for (int i = 0; i < C; ++i) {
      if (keep[i] == 1.0f) idx_host[my + nk++] = i;
      else if (keep[i] != 0.0f) binary = false;   // (a caller's scale vector that is no keep vector: the dense path multiplies by it)
    }
    if (!binary) continue;
    for (int i = nk; i < C; ++i) idx_host[my + i] = -1;
    const int nkM = std::min(C, (nk + 63) / 64 * 64), nkK = std::min(C, (nk + 15) / 16 * 16);
    if (nk == 0 || nkK >= C) continue;                       // nothing to leave out (or nothing kept: the dense path handles the zeros)
    if (!conv_x3_eligible(c0.Cin, nkM, 3) || !conv_x3_eligible(nkK, c1.Cout, 3) || !conv_x3_eligible(c1.Cout, nkM, 3) ||
        (b > 0 && !conv_x3_eligible(nkK, c0.Cin, 3)) || !conv_wgradx_eligible(nkM, c1.Cout, 3) || !conv_wgradx_eligible(c0.Cin, nkM, 3))
      continue;
    blk.dc_on = true; blk.nk = nk; blk.nkM = nkM; blk.nkK = nkK; blk.dc_idx = idx_dev + my;
  }
  return FRCNN_OK;
}

// The step's pack-job table: the model's jobs, those of the compact blocks re-written for the kept filters / channels; one
// asynchronous copy brings it and the kept-channel tables over, one launch packs.
static int pack_compact(frcnn_model* m, const float* w, bool f16, hipStream_t s) {
  const unsigned slot = m->dc_step % frcnn_model::DC_RING;
  ++m->dc_step;
  char* hslot = m->dc_pin.p + (size_t)slot * m->dc_slot_bytes;
  char* dslot = (char*)m->dc_dev.p + (size_t)slot * m->dc_slot_bytes;
  const Span& train = m->packs.x3_train[f16];
  const PackXJob* src = m->packs.x3.host_at(train);   // the model's training pack jobs (plain | fp16 form)
  PackXJob* jobs = (PackXJob*)hslot;
  int n = 0;
  for (int i = 0; i < train.n; ++i) {
    PackXJob j = src[i];
    const int ci = m->packs.x3_conv[i];
    if (ci < 0 && !m->head_x3_fresh) continue;   // an anchor net's pack in a pass that runs the anchor nets sparse
    if (ci >= 0) {
      const Conv& c = m->convs[ci];
      const Block& blk = m->blocks[c.block];
      if (blk.dc_on && c.step <= 1) {
        // (b, 0): filters gathered -- forward M = nkM, input gradient K = nkK;  (b, 1): channels gathered -- forward K = nkK,
        // input gradient M = nkM.  Entries beyond the kept ones are -1: rows / channels of zeros.
        PackXJob g;
        if (c.step == 0) {
          const int O = j.mode == 0 ? blk.nkM : blk.nkK;
          g = j.mode == 0 ? conv_x3_pack_job(c.w_off, O, c.Cin, c.k, 0, c.wx.p, c.Ho, c.Wo) : conv_x3_pack_job(c.w_off, O, c.Cin, c.k, 1, c.wxd.p, c.H, c.W);
          g.oidx = blk.dc_idx; g.Cs = c.Cin;
          if (j.mode == 0) { g.bias_off = c.b_off; g.bias_dst = blk.dc_bias.f(); }
        } else {
          const int C = j.mode == 0 ? blk.nkK : blk.nkM;
          g = j.mode == 0 ? conv_x3_pack_job(c.w_off, c.Cout, C, c.k, 0, c.wx.p, c.Ho, c.Wo) : conv_x3_pack_job(c.w_off, c.Cout, C, c.k, 1, c.wxd.p, c.H, c.W);
          g.cidx = blk.dc_idx; g.Cs = c.Cin;
        }
        g.amax = j.amax; g.amax_w = j.amax_w;
        j = g;
      }
    }
    jobs[n++] = j;
  }
  const int grid = conv_x3_pack_assign_blocks(jobs, n);
  FR_HIP(hipMemcpyAsync(dslot, hslot, m->dc_slot_bytes, hipMemcpyHostToDevice, s));
  FR_TRY(m->dc_ev[slot].record(s));
  FR_TRY(conv_x3_pack_multi(w, (const PackXJob*)dslot, n, grid, s));
  return FRCNN_OK;
}

static int pnet_forward_impl(frcnn_model* m, const float* w, const float* img, int H, int W, int training,
                             const float* const* drop_masks, unsigned long long seed, void* stream, bool async_heads) {
  hipStream_t s = S(stream);
  FR_TRY(join_side(m, s));   // (anchor nets of an abandoned asynchronous forward still read the model's buffers)
  if (H != m->H || W != m->W) FR_TRY(ensure_shapes(m, H, W));
  m->training = training;
  m->heads_begun = false; m->heads_joined = false; m->loss_pending = false;
  const bool use_side = side_enabled();
  async_heads = async_heads && use_side && training;
  // training through the objective: the anchor nets wait for the call that knows the sampled positions (heads.hip)
  m->heads_deferred = async_heads && sparse_heads_on() && !deterministic() && m->heads.size() <= 4;
  m->heads_sparse_fwd = false; m->heads_gin = false;
  m->last_w = w;
  if (use_side && !m->heads_deferred) { FR_TRY(ensure_side(m)); FR_TRY(ensure_head_streams(m)); }
  // SpatialDropout scales (device-drawn ones: one launch for all blocks)
  DropoutJobs dj;
  dj.n = 0;
  for (size_t b = 0; b < m->blocks.size(); ++b) {
    Block& blk = m->blocks[b];
    if (!blk.has_drop) continue;
    int C = m->d.filters[b];
    if (!training) {
      FR_TRY(fill_value(blk.scale.f(), C, 1.0f - blk.p_drop, s));  // evaluate(): x(1-p) [ext]
    } else if (drop_masks && drop_masks[b]) {
      FR_HIP(hipMemcpyAsync(blk.scale.p, drop_masks[b], (size_t)C * 4, hipMemcpyDeviceToDevice, s));
    } else {
      dj.ptr[dj.n] = blk.scale.f(); dj.C[dj.n] = C; dj.p[dj.n] = blk.p_drop; dj.seed[dj.n] = seed * 131 + b;
      ++dj.n;
    }
  }
  FR_TRY(dropout_channel_masks(dj, s));
  FR_TRY(plan_compact(m, training, drop_masks, seed));
  // weights change every optimiser step: refresh the packed copies (one table-driven launch each).  Option static_weights: an
  // evaluate-mode pass re-uses the packs of the previous evaluate-mode pass with the same weight vector -- the host's promise that
  // it has not written the weights in between (a training-mode pass, a shape change and every frcnn_set_option("static_weights", v)
  // call drop them).
  m->head_packs_fresh = false;
  const bool f16 = m->packs.f16();
  const bool reuse = !training && g_static_weights && m->eval_packs_gen == g_static_gen && m->eval_packs_w == w && m->f16_packed == f16;
  m->f16_packed = f16;
  std::fill(m->am_live.begin(), m->am_live.end(), 0);
  // ... or every owner's packs were renewed from this weight vector since the last pass (frcnn_pnet_refresh_packs: the update
  // ran beside the previous backward pass).  One-shot: the promise covers the pass that consumes it.
  const bool fresh = training && !m->packs.groups.empty() && m->fresh_mask == (1u << m->packs.groups.size()) - 1 && m->fresh_w == w &&
                     m->fresh_f16 == f16 && !any_compact(m);   // (a compact block's packs depend on the step's keep vector)
  m->fresh_mask = 0;
  if (!reuse && !fresh) {
    // (a training pass that leaves the anchor nets to the sparse path packs nothing of theirs: frcnn_model::head_x3_fresh)
    const PackTables& pt = m->packs;
    const bool skip_heads = training && m->heads_deferred && any_compact(m) && pt.am_bb.n > 0;
    m->head_x3_fresh = !skip_heads;
    FR_TRY(run_packs(m, w, skip_heads ? pt.pk_bb : training ? pt.pk_train : pt.pk_fwd, s));
    if (f16) {   // the weight tensors' magnitudes first: their packs are scaled by them
      FR_TRY(run_amax(m, w, skip_heads ? pt.am_bb : pt.am_all, s));
      m->weights_live(!skip_heads);
    }
    if (training && any_compact(m))
      FR_TRY(pack_compact(m, w, f16, s));   // the step's own table: the compact blocks' jobs gather the kept filters / channels
    else
      FR_TRY(run_x3_packs(m, w, training ? pt.x3_train[f16] : pt.x3_fwd[f16], s));
  }
  m->eval_packs_gen = training ? -1 : g_static_gen;
  m->eval_packs_w = w;
  FR_TRY(m->img.ensure((size_t)3 * H * W * 4));
  FR_HIP(hipMemcpyAsync(m->img.p, img, (size_t)3 * H * W * 4, hipMemcpyDeviceToDevice, s));
  const float* cur = m->img.f();
  const float* cur_slope = nullptr;
  const float* cur_scale = nullptr;
  const float* cur_am = nullptr;   // magnitude scalar of `cur` (fp16 form)
  for (size_t b = 0; b < m->blocks.size(); ++b) {
    Block& blk = m->blocks[b];
    bool pooled_in_conv = false;
    for (int st = 0; st < blk.nconv; ++st) {
      Conv& c = m->convs[blk.first_conv + st];
      const bool last = st == blk.nconv - 1;
      // the block's max pool rides in the epilogue of its last convolution when that launch is a single K split
      IgemmPool pl = {blk.pooled.f(), (unsigned char*)blk.pidx.p, w + c.a_off,
                      (st == 0 && blk.has_drop) ? blk.scale.f() : nullptr, f16 ? m->rec(blk.am) : nullptr};
      // fp16 form: the next convolution reads c.x scaled by its largest magnitude, which the launch that writes c.x records
      const bool want_am = f16 && !last && m->convs[blk.first_conv + st + 1].x_f;
      if (c.x_f && blk.dc_on && st <= 1) {
        // compact block: the first convolution computes its kept filters only (output stored compact), the second reads the
        // kept channels only -- their dropout scale is 1
        const int cin = st == 0 ? c.Cin : blk.nkK, mo = st == 0 ? blk.nkM : c.Cout;
        FR_TRY(conv_x3(cur, cin, c.H, c.W, cur_slope, nullptr, c.wx.p, st == 0 ? blk.dc_bias.f() : w + c.b_off, mo, c.k, c.pad, c.x.f(),
                       OUT_STORE, 0, s, 0, nullptr, f16 ? cur_am : nullptr, f16 ? m->amax_ws.f() + c.am : nullptr,
                       want_am ? m->rec_w(c.am) : nullptr));
      } else if (c.x_f)
        FR_TRY(conv_x3(cur, c.Cin, c.H, c.W, cur_slope, cur_scale, c.wx.p, w + c.b_off, c.Cout, c.k, c.pad, c.x.f(), OUT_STORE, 0, s, 0,
                       nullptr, f16 ? cur_am : nullptr, f16 ? m->amax_ws.f() + c.am : nullptr, want_am ? m->rec_w(c.am) : nullptr));
      else
        FR_TRY(conv_igemm(cur, c.Cin, c.H, c.W, cur_slope, cur_scale, c.wf.f(), w + c.b_off, c.Cout, c.k, c.pad,
                          c.x.f(), OUT_STORE, 0, s, 0, last ? &pl : nullptr, last ? &pooled_in_conv : nullptr));
      if (pooled_in_conv && pl.amax) m->am_live[blk.am] = 1;   // (the launch took pl and kept the pooled map's record)
      if (want_am) {
        if (!c.x_f) FR_TRY(tensor_absmax(c.x.f(), (long)c.Cout * c.Ho * c.Wo, m->rec_w(c.am), s));   // (the fp32 kernel keeps no record)
        cur_am = m->rec(c.am);
      }
      cur = c.x.f();
      cur_slope = w + c.a_off;
      cur_scale = (st == 0 && blk.has_drop) ? blk.scale.f() : nullptr;  // model_utilities.lua:20
    }
    const Conv& lc = m->convs[blk.first_conv + blk.nconv - 1];
    if (!pooled_in_conv)
      FR_TRY(maxpool_act_forward(cur, lc.Cout, lc.Ho, lc.Wo, cur_slope, cur_scale, blk.pooled.f(),
                                 (unsigned char*)blk.pidx.p, s, f16 ? m->rec_w(blk.am) : nullptr));
    // (pooled inside the fp32 kernel of the first layer: that launch kept the pooled map's record)
    cur = blk.pooled.f();
    cur_slope = nullptr;
    cur_scale = nullptr;
    cur_am = f16 ? m->rec(blk.am) : nullptr;   // the pooled map feeds the next block and the anchor nets on it
    // anchor nets on an earlier block's map run beside the following blocks, each on its own stream
    if (use_side && b + 1 < m->blocks.size() && !m->heads_deferred) {
      FR_TRY(ensure_side(m));
      for (size_t i = 0; i < m->heads.size(); ++i) {
        Head& h = m->heads[i];
        if (h.input != (int)b) continue;
        FR_TRY(fork_to(m, s, head_stream(m, i), 16 + i));
        FR_TRY(head_forward(m, h, w, head_stream(m, i), head_slot(m, i)));
      }
    }
  }
  // heads on the LAST block's map: the heaviest stays on the caller's stream, the others run beside it
  if (!m->heads_deferred) {
    const int last = (int)m->blocks.size() - 1;
    int heavy = -1;
    for (size_t i = 0; i < m->heads.size(); ++i)
      if ((!use_side || m->heads[i].input == last) && (heavy < 0 || m->heads[i].c3.k > m->heads[heavy].c3.k)) heavy = (int)i;
    if (async_heads) heavy = -1;   // the caller's stream goes on with the last map; every anchor net stays off it
    if (use_side) FR_TRY(ensure_side(m));
    for (size_t i = 0; use_side && i < m->heads.size(); ++i) {
      if (m->heads[i].input != last || (int)i == heavy) continue;
      FR_TRY(fork_to(m, s, head_stream(m, i), 16 + i));
      FR_TRY(head_forward(m, m->heads[i], w, head_stream(m, i), head_slot(m, i)));
    }
    for (size_t i = 0; i < m->heads.size(); ++i)
      if ((int)i == heavy || (!use_side)) FR_TRY(head_forward(m, m->heads[i], w, s, 0));
  }
  if (use_side && !async_heads) FR_TRY(join_side(m, s));   // the caller's stream continues after every head is done
  return FRCNN_OK;
}

int frcnn_pnet_forward(frcnn_model* m, const float* w, const float* img, int H, int W, int training,
                       const float* const* drop_masks, unsigned long long seed, void* stream) {
  return pnet_forward_impl(m, w, img, H, W, training, drop_masks, seed, stream, false);
}

int frcnn_pnet_forward_async_heads(frcnn_model* m, const float* w, const float* img, int H, int W,
                                   const float* const* drop_masks, unsigned long long seed, void* stream) {
  return pnet_forward_impl(m, w, img, H, W, 1, drop_masks, seed, stream, true);
}

int frcnn_pnet_output(frcnn_model* m, int i, float** ptr, int* C, int* H, int* W) {
  FR_CHECK(m->H > 0, "pnet_output: call frcnn_pnet_forward first");
  FR_CHECK(i >= 1 && i <= (int)m->heads.size() + 1, "pnet_output: index %d out of range", i);
  if (i <= (int)m->heads.size()) {
    Head& h = m->heads[i - 1];
    *ptr = h.c1.x.f(); *C = HEAD_OUT; *H = h.c1.Ho; *W = h.c1.Wo;
  } else {
    Block& b = m->blocks.back();
    *ptr = b.pooled.f(); *C = m->d.filters[m->d.nblocks - 1]; *H = b.Hp; *W = b.Wp;
  }
  return FRCNN_OK;
}

int frcnn_model_debug_buffer(frcnn_model* m, int kind, int index, void** ptr, long long* bytes) {
  FR_CHECK(m && ptr && bytes, "frcnn_model_debug_buffer: NULL argument");
  const DevBuf* b = nullptr;
  size_t n = 0;
  switch (kind) {
    case 0: {
      FR_CHECK(index >= 0 && index < (int)m->convs.size() && m->H > 0, "debug_buffer: backbone convolution %d (after a forward pass)", index);
      const Conv& c = m->convs[index]; b = &c.x; n = (size_t)c.Cout * c.Ho * c.Wo * 4;
      const Block& k = m->blocks[c.block];
      if (k.dc_on && c.step == 0) {   // stored compact in this pass (Block::dc_on): laid out dense here, zeros where nothing was computed
        FR_HIP(hipDeviceSynchronize());
        FR_TRY(m->dbg_expand.ensure(n));
        FR_HIP(hipMemset(m->dbg_expand.p, 0, n));
        std::vector<int> idx(c.Cout);
        FR_HIP(hipMemcpy(idx.data(), k.dc_idx, (size_t)c.Cout * 4, hipMemcpyDeviceToHost));
        const size_t row = (size_t)c.Ho * c.Wo * 4;
        for (int i = 0; i < k.nk; ++i)
          FR_HIP(hipMemcpy((char*)m->dbg_expand.p + (size_t)idx[i] * row, (const char*)c.x.p + (size_t)i * row, row, hipMemcpyDeviceToDevice));
        b = &m->dbg_expand;
      }
    } break;
    case 4: {   // the SpatialDropout scale vector of block `index` in the last pass (a keep vector while training)
      FR_CHECK(index >= 0 && index < (int)m->blocks.size() && m->H > 0 && m->blocks[index].has_drop, "debug_buffer: block %d has no dropout", index);
      const Block& k = m->blocks[index]; b = &k.scale; n = (size_t)m->d.filters[index] * 4;
    } break;
    case 1: {
      FR_CHECK(index >= 0 && index < (int)m->blocks.size() && m->H > 0, "debug_buffer: block %d (after a forward pass)", index);
      const Block& k = m->blocks[index]; b = &k.pidx; n = (size_t)m->d.filters[index] * k.Hp * k.Wp;
    } break;
    case 2: {
      FR_CHECK(index >= 0 && index < (int)m->heads.size() && m->H > 0, "debug_buffer: anchor net %d (after a forward pass)", index);
      const Conv& c = m->heads[index].c3; b = &c.x; n = (size_t)c.Cout * c.Ho * c.Wo * 4;
      if ((m->heads_sparse_fwd || m->heads_deferred) && m->last_w) {
        // the training pass computed this map at the sampled positions only (heads.hip), or not yet: the dense convolution, now
        FR_HIP(hipDeviceSynchronize());
        if (!m->head_x3_fresh) { FR_TRY(refresh_group(m, m->last_w, (int)m->blocks.size(), nullptr)); m->head_x3_fresh = true; }
        FR_TRY(head_forward(m, m->heads[index], m->last_w, nullptr, 0));
        FR_HIP(hipDeviceSynchronize());
      }
    } break;
    case 3: {
      FR_CHECK(index >= 0 && index < (int)m->cls.size() && m->R > 0, "debug_buffer: classification layer %d (after frcnn_cnet_forward)", index);
      const ClsLayer& L = m->cls[index]; b = L.bn ? &L.pre : &L.lin; n = (size_t)m->R * L.n * 4;
    } break;
    case 7: case 11: {   // a backbone convolution's output / finished output gradient as stored (compact in a compact block)
      FR_CHECK(index >= 0 && index < (int)m->convs.size() && m->H > 0, "debug_buffer: backbone convolution %d (after a forward pass)", index);
      const Conv& c = m->convs[index];
      const Block& k = m->blocks[c.block];
      b = kind == 7 ? &c.x : &c.gx; n = (size_t)((k.dc_on && c.step == 0) ? k.nkM : c.Cout) * c.Ho * c.Wo * 4;
    } break;
    case 9: {
      FR_CHECK(index >= 0 && index < (int)m->blocks.size() && m->H > 0, "debug_buffer: block %d (after a forward pass)", index);
      const Block& k = m->blocks[index]; b = &k.pooled; n = (size_t)m->d.filters[index] * k.Hp * k.Wp * 4;
    } break;
    case 5: case 6: case 8: case 10: {   // magnitude records: only what the last pass wrote
      const int nc = (int)m->convs.size();
      int id = -1;
      FR_CHECK(m->H > 0, "debug_buffer: magnitude records exist after a forward pass");
      if (kind == 6) {
        FR_CHECK(index >= 0 && index < (int)m->blocks.size(), "debug_buffer: block %d out of range", index);
        id = m->blocks[index].am;
      } else if (kind == 10) {
        FR_CHECK(index >= 0 && index < nc + (int)m->heads.size(), "debug_buffer: weight tensor %d out of range", index);
        id = (index < nc ? m->convs[index].am : m->heads[index - nc].c3.am) + 2;
      } else {
        FR_CHECK(index >= 0 && index < nc, "debug_buffer: backbone convolution %d out of range", index);
        id = m->convs[index].am + (kind == 8 ? 1 : 0);
      }
      FR_CHECK(id >= 0 && id < (int)m->am_live.size() && m->am_live[id], "debug_buffer: the last pass kept no magnitude record of kind %d, index %d", kind, index);
      *ptr = m->rec(id); *bytes = (long long)AMAX_REC * 4;
      return FRCNN_OK;
    }
    default: FR_CHECK(false, "debug_buffer: unknown kind %d", kind);
  }
  FR_CHECK(b->p && b->bytes >= n, "debug_buffer: buffer not allocated yet");
  *ptr = b->p; *bytes = (long long)n;
  return FRCNN_OK;
}

int frcnn_pnet_delta(frcnn_model* m, int i, float** ptr) {
  FR_CHECK(m->H > 0, "pnet_delta: call frcnn_pnet_forward first");
  FR_CHECK(i >= 1 && i <= (int)m->heads.size() + 1, "pnet_delta: index %d out of range", i);
  *ptr = i <= (int)m->heads.size() ? m->heads[i - 1].delta.f() : m->delta_last.f();
  return FRCNN_OK;
}

int frcnn_pnet_set_sparse_deltas(frcnn_model* m, int head, const int* positions, int count) {
  FR_CHECK(head >= 1 && head <= (int)m->heads.size(), "pnet_set_sparse_deltas: head %d out of range", head);
  m->heads[head - 1].sp_pos = positions;
  m->heads[head - 1].sp_count = count;
  return FRCNN_OK;
}

int frcnn_pnet_zero_deltas(frcnn_model* m, void* stream) {
  FR_CHECK(m->H > 0, "pnet_zero_deltas: call frcnn_pnet_forward first");
  FR_TRY(fill_zero(m->zero_arena.p, m->delta_bytes, S(stream)));
  return FRCNN_OK;
}

// One anchor net's part of pnet:backward: gradients of its parameters, input gradient added into the pooled map's gradient
// buffer (nngraph fan-out; atomic adds -- several anchor nets feed the same map).  Runs on stream s with split-K workspace
// slot ws_slot.  *dense is set when the dense fallback was taken (no usable sparse hint).
static bool head_is_sparse(const Head& h) { return h.sp_count >= 0 && h.sp_count <= SPARSE_MAX_POS; }
// staged training: the anchor net's contribution to its input map's gradient is needed only while that block is trained
static bool head_needs_gin(const frcnn_model* m, const Head& h) { return h.input >= m->frozen_blocks; }
// ... and the pooled maps' gradient buffers (which the anchor nets add into) only while some block is
static bool backbone_trained(const frcnn_model* m) { return m->frozen_blocks < (int)m->blocks.size(); }

static int backward_head(frcnn_model* m, Head& h, const float* w, float* grad, hipStream_t s, int ws_slot) {
  Block& in = m->blocks[h.input];
  Conv &a = h.c3, &c = h.c1;
  const long hw1 = (long)c.Ho * c.Wo;
  if (head_is_sparse(h)) {
    // ---- sparse path: the same arithmetic restricted to the P positions where delta is non-zero
    const int P = h.sp_count;
    const int* pos = h.sp_pos;
    h.sp_count = -1; h.sp_pos = nullptr;   // one-shot hint
    if (P == 0) return FRCNN_OK;           // no example on this head: every gradient term is zero
    const int n = a.Cout, ckk = a.Cin * a.k * a.k;
    FR_TRY(h.spD.ensure((size_t)HEAD_OUT * SPARSE_MAX_POS * 4));
    FR_TRY(h.spHX.ensure((size_t)n * SPARSE_MAX_POS * 4));
    FR_TRY(h.spHY.ensure((size_t)n * SPARSE_MAX_POS * 4));
    FR_TRY(h.spGH.ensure((size_t)n * SPARSE_MAX_POS * 4));
    FR_TRY(h.spCol.ensure((size_t)ckk * SPARSE_MAX_POS * 4));
    FR_TRY(h.spDX.ensure((size_t)ckk * SPARSE_MAX_POS * 4));
    float *D = h.spD.f(), *HX = h.spHX.f(), *HY = h.spHY.f(), *GH = h.spGH.f(), *COL = h.spCol.f(), *DX = h.spDX.f();
    FR_TRY(gather_positions(h.delta.f(), HEAD_OUT, hw1, pos, P, D, nullptr, nullptr, s));
    FR_TRY(gather_positions(a.x.f(), n, hw1, pos, P, HX, w + a.a_off, HY, s));
    // the input-gradient path first (the backbone's backward pass waits for it), the parameter gradients after it:
    // GH[n][P] = W1^T[n][18] * D[18][P], then PReLU backward (+ bias / slope gradients of the k x k conv)
    FR_TRY(gemm_f32(w + c.w_off, 1, n, D, P, 1, GH, P, n, P, HEAD_OUT, OUT_STORE, nullptr, s, ws_slot));
    FR_TRY(act_backward(GH, HX, n, P, w + a.a_off, nullptr, GH, grad + a.b_off, grad + a.a_off, s));
    if (head_needs_gin(m, h)) {
      // DX[P][ckk] = GH^T[P][n] * W[n][ckk], scattered back into the pooled-map gradient
      FR_TRY(gemm_f32(GH, 1, P, w + a.w_off, ckk, 1, DX, ckk, P, ckk, n, OUT_STORE, nullptr, s, ws_slot));
      FR_TRY(col2im_positions_add(DX, a.Cin, a.H, a.W, a.k, a.Wo, pos, P, in.gpooled.f(), s));
    }
    if (h.stream && s == h.stream) {   // (on its own stream: see Head::gin_done)
      FR_TRY(h.gin_done.record(s));
      h.gin_recorded = true;
    }
    // 1x1 conv: gW1[18][n] += D[18][P] * HY[n][P]^T ; gb1 += rowsum(D)
    FR_TRY(gemm_f32(D, P, 1, HY, 1, P, grad + c.w_off, n, HEAD_OUT, n, P, OUT_ADD, nullptr, s, ws_slot));
    FR_TRY(channel_sum(D, HEAD_OUT, P, grad + c.b_off, s));
    // k x k conv: gW[n][ckk] += GH[n][P] * COL[P][ckk]
    FR_TRY(im2col_positions(in.pooled.f(), a.Cin, a.H, a.W, a.k, a.Wo, pos, P, COL, s));
    FR_TRY(gemm_f32(GH, P, 1, COL, ckk, 1, grad + a.w_off, ckk, n, ckk, P, OUT_ADD, nullptr, s, ws_slot));
    return FRCNN_OK;
  }
  h.sp_count = -1; h.sp_pos = nullptr;
  if (!m->head_packs_fresh) {   // dense fallback: bring the heads' input-gradient packs up to date
    FR_TRY(run_packs(m, w, m->packs.pk_heads, s));
    m->head_packs_fresh = true;
  }
  // 1x1 conv: accGradParameters + updateGradInput
  FR_TRY(conv_wgrad(a.x.f(), c.Cin, c.H, c.W, w + a.a_off, nullptr, h.delta.f(), HEAD_OUT, 1, 0, grad + c.w_off, m->wg_ws.p, m->wg_ws.bytes, s));
  FR_TRY(channel_sum(h.delta.f(), HEAD_OUT, hw1, grad + c.b_off, s));
  double f1 = 2.0 * HEAD_OUT * c.Cin * (double)hw1;
  FR_TRY(conv_igemm(h.delta.f(), HEAD_OUT, c.Ho, c.Wo, nullptr, nullptr, c.wd.f(), nullptr, c.Cin, 1, 0, a.gx.f(),
                    OUT_STORE, f1, s, ws_slot));
  // PReLU backward of the head (+ bias gradient of the k x k conv)
  FR_TRY(act_backward(a.gx.f(), a.x.f(), a.Cout, (long)a.Ho * a.Wo, w + a.a_off, nullptr, a.gx.f(),
                      grad + a.b_off, grad + a.a_off, s));
  FR_TRY(conv_wgrad(in.pooled.f(), a.Cin, a.H, a.W, nullptr, nullptr, a.gx.f(), a.Cout, a.k, 0, grad + a.w_off, m->wg_ws.p, m->wg_ws.bytes, s));
  if (!head_needs_gin(m, h)) return FRCNN_OK;
  double f3 = 2.0 * a.Cout * a.Cin * a.k * a.k * (double)a.Ho * a.Wo;
  FR_TRY(conv_igemm(a.gx.f(), a.Cout, a.Ho, a.Wo, nullptr, nullptr, a.wd.f(), nullptr, a.Cin, a.k, a.k - 1,
                    in.gpooled.f(), OUT_ADD, f3, s, ws_slot));  // nngraph fan-out: gradients add up
  return FRCNN_OK;
}

// every anchor net on ONE stream, one after the other (serial mode, and the fallback of frcnn_pnet_backward)
static int backward_heads(frcnn_model* m, const float* w, float* grad, hipStream_t s, int ws_slot) {
  for (auto& h : m->heads) FR_TRY(backward_head(m, h, w, grad, s, ws_slot));
  return FRCNN_OK;
}

// The anchor nets' backward pass off the caller's stream: the side stream holds whatever must precede it (its last
// event = chain_ev); every anchor net with a sparse hint then runs on its own stream beside the others, the dense
// fallback (shared weight-gradient workspace) stays on the side stream.
static int backward_heads_fanout(frcnn_model* m, const float* w, float* grad) {
  FR_TRY(ensure_head_streams(m));
  if (backbone_trained(m)) FR_TRY(fill_zero((char*)m->zero_arena.p + m->delta_bytes, m->gpool_bytes, m->side));
  FR_TRY(m->chain_ev.record(m->side));
  for (auto& h : m->heads) h.gin_recorded = false;
  std::vector<char> own(m->heads.size(), 0);   // (the hint is consumed by backward_head: decide before calling it)
  for (size_t i = 0; i < m->heads.size(); ++i) own[i] = m->heads[i].stream && head_is_sparse(m->heads[i]);
  // A dense-fallback net adds into the pooled-map gradient with plain read-modify-writes and uses the shared weight-gradient
  // workspace, while the sparse nets add into the same map with atomics from their own streams: nothing orders the two
  // groups, so as soon as ONE net is dense every net runs on the side stream, one after the other.
  bool any_dense = false;
  for (size_t i = 0; i < m->heads.size(); ++i) any_dense = any_dense || !head_is_sparse(m->heads[i]);
  // Deterministic mode: the order-independent forms (the gathering col2im, in-order folds) assume ONE writer of the shared
  // pooled-map gradient at a time.
  if (any_dense || deterministic()) std::fill(own.begin(), own.end(), 0);
  for (size_t i = 0; i < m->heads.size(); ++i) {
    Head& h = m->heads[i];
    if (!own[i]) continue;
    FR_TRY(m->chain_ev.wait(h.stream));
    FR_TRY(backward_head(m, h, w, grad, h.stream, head_slot(m, i)));
  }
  for (size_t i = 0; i < m->heads.size(); ++i)
    if (!own[i]) FR_TRY(backward_head(m, m->heads[i], w, grad, m->side, 1));
  return FRCNN_OK;
}

// The forward part a training pass deferred (frcnn_model::heads_deferred), as the dense convolutions after all: every anchor net
// on its own stream behind everything queued on `s` (the pooled maps are final there).
static int heads_forward_dense(frcnn_model* m, const float* w, hipStream_t s) {
  FR_TRY(ensure_side(m));
  FR_TRY(ensure_head_streams(m));
  if (!m->head_x3_fresh) {   // the pass packed nothing of the anchor nets (it meant to run them sparse)
    FR_TRY(refresh_group(m, w, (int)m->blocks.size(), s));
    m->head_x3_fresh = true;
  }
  for (size_t i = 0; i < m->heads.size(); ++i) {
    FR_TRY(fork_to(m, s, head_stream(m, i), 16 + i));
    FR_TRY(head_forward(m, m->heads[i], w, head_stream(m, i), head_slot(m, i)));
  }
  m->heads_deferred = false;
  return FRCNN_OK;
}

static bool heads_all_sparse(const frcnn_model* m) {
  for (auto& h : m->heads) if (!head_is_sparse(h)) return false;
  return !m->heads.empty() && m->heads.size() <= 4;
}

// The job table of the sparse path: the anchor nets that have sampled positions in this pass (heads_add_job skips the others
// and plans the K splits).  Staged training: a net whose input block is frozen has no gin.
static int heads_jobs(frcnn_model* m, const float* w, float* grad, HeadJobs& g) {
  g.n = 0;
  for (auto& h : m->heads) {
    const int P = h.sp_count;
    if (P <= 0) continue;
    Block& in = m->blocks[h.input];
    Conv &a = h.c3, &c = h.c1;
    const size_t n = (size_t)a.Cout, ckk = (size_t)a.Cin * a.k * a.k, cap = SPARSE_MAX_POS;
    FR_TRY(h.spD.ensure((size_t)HEAD_OUT * cap * 4)); FR_TRY(h.spOut.ensure((size_t)HEAD_OUT * cap * 4));
    FR_TRY(h.spHX.ensure(n * cap * 4)); FR_TRY(h.spHY.ensure(n * cap * 4)); FR_TRY(h.spGH.ensure(n * cap * 4));
    FR_TRY(h.spCol.ensure(ckk * cap * 4)); FR_TRY(h.spDX.ensure(ckk * cap * 4));
    FR_TRY(h.spSlab.ensure(n * 4096 * 4));   // (splits * P <= 4096 whatever P and n: allocated once)
    HeadJob j;
    j.Cin = a.Cin; j.H = a.H; j.W = a.W; j.k = a.k; j.Ho = a.Ho; j.Wo = a.Wo; j.n = a.Cout;
    j.P = P; j.pos = h.sp_pos;
    j.in = in.pooled.f(); j.gin = head_needs_gin(m, h) ? in.gpooled.f() : nullptr;
    j.bias3 = w + a.b_off; j.slope = w + a.a_off; j.bias1 = w + c.b_off;
    j.gbias3 = grad ? grad + a.b_off : nullptr; j.gslope = grad ? grad + a.a_off : nullptr; j.gbias1 = grad ? grad + c.b_off : nullptr;
    j.w3 = w + a.w_off; j.w1 = w + c.w_off;
    j.gw3 = grad ? grad + a.w_off : nullptr; j.gw1 = grad ? grad + c.w_off : nullptr;
    j.out = c.x.f(); j.delta = h.delta.f();
    j.COL = h.spCol.f(); j.HX = h.spHX.f(); j.HY = h.spHY.f(); j.OUT = h.spOut.f(); j.D = h.spD.f(); j.GH = h.spGH.f(); j.DX = h.spDX.f();
    j.hx_slab = h.spSlab.f(); j.hx_splits = 0;
    FR_TRY(heads_add_job(g, j, 0, n * 4096));
  }
  return FRCNN_OK;
}

// backward at the sampled positions (heads.hip): the model's part is the event between the chain's two halves and the hints
static int heads_sparse_backward(frcnn_model* m, const HeadJobs& g, hipStream_t s) {
  if (g.n == 0) return FRCNN_OK;
  FR_TRY(heads_chain_backward_input(g, s));
  FR_TRY(m->heads_gin_ev.record(s));                   // what the backbone's backward pass waits for; the parameter gradients follow
  m->heads_gin = true;
  FR_TRY(heads_chain_backward_params(g, s));
  for (auto& h : m->heads) { h.sp_count = -1; h.sp_pos = nullptr; }   // one-shot hints
  return FRCNN_OK;
}

int frcnn_pnet_backward_heads_begin(frcnn_model* m, const float* w, float* grad, void* stream) {
  hipStream_t s = S(stream);
  FR_CHECK(m->H > 0 && m->training, "pnet_backward_heads_begin: needs a preceding training-mode forward");
  if (!side_enabled() || m->heads_begun || !m->train_heads) return FRCNN_OK;   // frcnn_pnet_backward does everything
  if (m->heads_deferred) FR_TRY(heads_forward_dense(m, w, s));   // (this entry point has no sparse forward: the outputs were the caller's to read)
  FR_TRY(fork_side(m, s, m->blocks.size() + 1));             // delta_outputs[1..nheads] are final on s
  FR_TRY(join_heads(m, m->side));                            // (anchor nets of an asynchronous forward still in flight)
  FR_TRY(backward_heads_fanout(m, w, grad));
  m->heads_begun = true;
  return FRCNN_OK;
}

// Staged training with the anchor nets frozen: the losses are queued, nothing of the anchor nets' backward pass is.  The pass counts
// as begun (frcnn_pnet_backward joins the side stream, which holds the losses) with no input-gradient contribution recorded.
static int heads_frozen_begun(frcnn_model* m) {
  for (auto& h : m->heads) { h.sp_count = -1; h.sp_pos = nullptr; h.gin_recorded = false; }   // (one-shot hints, unused)
  m->heads_gin = false;
  m->heads_begun = true;
  return FRCNN_OK;
}

int frcnn_pnet_anchor_loss_begin(frcnn_model* m, const float* w, float* grad, const int* ex_idx, const double* ex_anchor,
                                 const double* ex_roi, const int* ex_class, int npos, int nneg, int bgclass,
                                 double* ex_loss, float* crtarget, float* cctarget, double* acc, void* stream) {
  hipStream_t s = S(stream);
  FR_CHECK(m->H > 0 && m->training, "pnet_anchor_loss_begin: needs a preceding training-mode forward");
  FR_CHECK(m->heads.size() <= 4, "pnet_anchor_loss_begin: at most 4 anchor nets");
  FR_CHECK(!m->heads_begun, "pnet_anchor_loss_begin: the anchor nets' backward pass has already been started");
  RpnLayers L;
  float* deltas[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int l = 0; l < 4; ++l) {
    const bool have = l < (int)m->heads.size();
    L.map[l] = have ? m->heads[l].c1.x.f() : nullptr;
    L.H[l] = have ? m->heads[l].c1.Ho : 0; L.W[l] = have ? m->heads[l].c1.Wo : 0;
    deltas[l] = have ? m->heads[l].delta.f() : nullptr;
  }
  const int E = npos + nneg;
  if (!side_enabled()) {   // serial: the losses on the caller's stream, the backward part left to frcnn_pnet_backward
    FR_TRY(rpn_loss(L, deltas, ex_idx, ex_anchor, ex_roi, ex_class, npos, nneg, bgclass, ex_loss, crtarget, cctarget, s));
    FR_TRY(loss_accumulate(ex_loss, E, acc, s));
    return FRCNN_OK;
  }
  if (m->heads_deferred && heads_all_sparse(m)) {
    // The sparse path (heads.hip): forward at the sampled positions, the losses, the backward part -- one chain of grouped
    // launches on the side stream, behind everything queued on `s` (pooled maps, example tables, zeroed delta buffers)
    HeadJobs g;
    FR_TRY(heads_jobs(m, w, grad, g));
    FR_TRY(fork_side(m, s, m->blocks.size() + 1));
    FR_TRY(heads_chain_forward(g, m->side));
    m->heads_deferred = false; m->heads_sparse_fwd = true;
    FR_TRY(rpn_loss(L, deltas, ex_idx, ex_anchor, ex_roi, ex_class, npos, nneg, bgclass, ex_loss, crtarget, cctarget, m->side));
    FR_TRY(loss_accumulate(ex_loss, E, acc, m->side));
    FR_TRY(m->loss_ev.record(m->side));
    m->loss_pending = true;
    if (!m->train_heads) return heads_frozen_begun(m);   // staged training: the chain stops after the losses
    if (backbone_trained(m)) FR_TRY(fill_zero((char*)m->zero_arena.p + m->delta_bytes, m->gpool_bytes, m->side));
    FR_TRY(heads_sparse_backward(m, g, m->side));
    m->heads_begun = true;
    return FRCNN_OK;
  }
  if (m->heads_deferred) FR_TRY(heads_forward_dense(m, w, s));   // more positions than the sparse path takes: the dense convolutions after all
  FR_TRY(fork_side(m, s, m->blocks.size() + 1));   // example tables and zeroed delta buffers are final on s
  FR_TRY(join_heads(m, m->side));                  // the anchor nets' outputs (each on its own stream) are final
  FR_TRY(rpn_loss(L, deltas, ex_idx, ex_anchor, ex_roi, ex_class, npos, nneg, bgclass, ex_loss, crtarget, cctarget, m->side));
  FR_TRY(loss_accumulate(ex_loss, E, acc, m->side));
  FR_TRY(m->loss_ev.record(m->side));
  m->loss_pending = true;
  if (!m->train_heads) return heads_frozen_begun(m);
  FR_TRY(backward_heads_fanout(m, w, grad));
  m->heads_begun = true;
  return FRCNN_OK;
}

int frcnn_pnet_anchor_loss_wait(frcnn_model* m, void* stream) {
  if (m->loss_pending) {
    FR_TRY(m->loss_ev.wait(S(stream)));
    m->loss_pending = false;
  }
  return FRCNN_OK;
}

int frcnn_pnet_backward_heads_join(frcnn_model* m, void* stream, int* joined) {
  hipStream_t s = S(stream);
  if (joined) *joined = 0;
  if (!m->heads_begun) return FRCNN_OK;   // nothing was started: frcnn_pnet_backward computes the anchor nets' part
  if (!m->heads_joined) {
    FR_TRY(join_heads(m, s));
    FR_TRY(join_side_now(m, s));
    m->heads_joined = true;   // frcnn_pnet_backward will not wait again
  }
  if (joined) *joined = 1;
  return FRCNN_OK;
}

// After frcnn_pnet_backward has been queued: `stream` waits until the caller's stream has joined the anchor nets and begun the
// backbone's backward pass -- the stretch of the step that is bound by the matrix cores, beside which bandwidth-bound work
// (the update of slices that are final already) costs least.  Everything the caller's stream ran before it is final too.
int frcnn_pnet_wait_backward_begun(frcnn_model* m, void* stream) {
  FR_CHECK(m->update_armed && m->bwd_ev.recorded() && m->block_ev_valid,
           "pnet_wait_backward_begun: call frcnn_model_update_stream before the pass and frcnn_pnet_backward first");
  return m->bwd_ev.wait(S(stream));
}

// After frcnn_pnet_backward has been queued: `stream` waits until the anchor nets' whole backward pass -- their parameter
// gradients included, which may still be running beside the backbone's pass -- is over: their slice may then be updated.
int frcnn_pnet_wait_heads_done(frcnn_model* m, void* stream) {
  FR_CHECK(m->block_ev_valid, "pnet_wait_heads_done: call frcnn_pnet_backward first");
  for (auto& h : m->heads)
    if (h.stream) FR_TRY(h.done.wait(S(stream)));
  if (m->side) {   // (the sparse training path runs the anchor nets on the side stream: everything queued there so far)
    FR_TRY(ensure_update_stream(m));
    FR_TRY(chain(m->side, S(stream), m->upd_ev));
  }
  return FRCNN_OK;
}

// Stream `stream` waits until block `block`'s slice of the flat vectors may be UPDATED: its parameter gradients are final (block_ev)
// and the caller's stream has queued -- hence, in stream order, finished -- the last launch that reads the block's weights, its
// packs or its weight-magnitude scalars (the input-gradient launch of the block's first convolution).
int frcnn_pnet_wait_block_done(frcnn_model* m, int block, void* stream) {
  FR_CHECK(block >= 1 && block <= (int)m->blocks.size(), "pnet_wait_block_done: block %d out of range", block);
  // (the read events are recorded by a pass that found the update stream armed)
  FR_CHECK(m->update_armed && m->block_ev_valid && m->block_rd_ev[block - 1].recorded(),
           "pnet_wait_block_done: call frcnn_model_update_stream before the pass and frcnn_pnet_backward first");
  FR_TRY(m->block_ev[block - 1].wait(S(stream)));
  return m->block_rd_ev[block - 1].wait(S(stream));
}

// Renews the training packs of one owner (group = 0-based backbone block, or the number of blocks for the anchor nets) from the
// weight vector w on `stream`: what the prologue of frcnn_pnet_forward does for the whole model, for the slice whose update has
// just been queued on the same stream.  When every group has been renewed from the vector the next training-mode forward is
// given, that forward skips its prologue.  The caller promises that nothing writes w between this call and that forward except
// updates followed by their own refresh; frcnn_pnet_invalidate_packs withdraws the promise.
static int refresh_group(frcnn_model* m, const float* w, int group, hipStream_t s) {
  const bool f16 = m->packs.f16();
  const PackTables::Group& G = m->packs.groups[group];
  FR_TRY(run_packs(m, w, G.pk, s));
  if (f16) FR_TRY(run_amax(m, w, G.am, s));
  return run_x3_packs(m, w, G.x3[f16], s);
}
int frcnn_pnet_refresh_packs(frcnn_model* m, const float* w, int group, void* stream) {
  FR_CHECK(m->H > 0, "pnet_refresh_packs: call frcnn_pnet_forward first");
  FR_CHECK(group >= 0 && group < (int)m->packs.groups.size(), "pnet_refresh_packs: group %d out of range", group);
  const bool f16 = m->packs.f16();
  if (m->fresh_mask && (m->fresh_w != w || m->fresh_f16 != f16)) m->fresh_mask = 0;
  FR_TRY(refresh_group(m, w, group, S(stream)));
  if (group == (int)m->blocks.size()) m->head_x3_fresh = true;
  m->fresh_mask |= 1u << group; m->fresh_w = w; m->fresh_f16 = f16;
  return FRCNN_OK;
}

int frcnn_pnet_invalidate_packs(frcnn_model* m) {
  m->fresh_mask = 0;
  return FRCNN_OK;
}

int frcnn_pnet_wait_block_gradients(frcnn_model* m, int block, void* stream) {
  FR_CHECK(block >= 1 && block <= (int)m->blocks.size(), "pnet_wait_block_gradients: block %d out of range", block);
  FR_CHECK(m->block_ev_valid, "pnet_wait_block_gradients: call frcnn_pnet_backward first");
  return m->block_ev[block - 1].wait(S(stream));
}

// block b's weights, packs and weight magnitudes have had their last reader on the caller's stream s
static int record_block_read(frcnn_model* m, int b, hipStream_t s) {
  return m->update_armed ? m->block_rd_ev[b].record(s) : FRCNN_OK;
}
// block b's parameter gradients are final at this point of stream s, and its weights have been read for the last time there
static int mark_block_done(frcnn_model* m, int b, hipStream_t s) {
  FR_TRY(m->block_ev[b].record(s));
  return record_block_read(m, b, s);
}

// The anchor nets' part of frcnn_pnet_backward: the caller's stream s waits for what the backbone's pass needs from them (or
// computes it, when nobody has started it).  *heads_tail: anchor nets are still computing their parameter gradients on streams
// of their own, to be joined at the end of the pass.
static int join_anchor_nets_for_backbone(frcnn_model* m, const float* w, float* grad, hipStream_t s, bool* heads_tail) {
  *heads_tail = false;
  if (m->heads_begun) {   // started by frcnn_pnet_backward_heads_begin: wait for the side stream
    if (!m->heads_joined) {
      // What the backbone's pass needs from an anchor net is its contribution to the pooled map's gradient; a net on a stream
      // of its own marks that point (Head::gin_done) and goes on with its parameter gradients beside the backbone's pass.
      if (m->heads_gin) {   // the sparse path's one chain on the side stream: its input-gradient part, the rest at the end
        FR_TRY(m->heads_gin_ev.wait(s));
        *heads_tail = true;
      }
      for (auto& h : m->heads) {
        if (!h.stream || m->heads_gin) continue;
        if (h.gin_recorded) {
          FR_TRY(h.gin_done.wait(s));
          *heads_tail = true;
        } else {
          FR_TRY(chain(h.stream, s, h.done));
        }
      }
      if (!m->heads_gin) FR_TRY(join_side_now(m, s));
    }
    m->heads_begun = false; m->heads_joined = false; m->side_busy = false;
  } else if (!m->train_heads) {   // staged training, anchor nets frozen: their deltas are not back-propagated
    for (auto& h : m->heads) { h.sp_count = -1; h.sp_pos = nullptr; }
    m->heads_deferred = false;
    FR_TRY(join_side(m, s));
  } else {
    if (m->heads_deferred) {   // nobody asked for the anchor nets' outputs; their backward part below needs the forward part unless no net has a position
      bool any = false;
      for (auto& h : m->heads) any = any || h.sp_count != 0;
      if (any) FR_TRY(heads_forward_dense(m, w, s));
      m->heads_deferred = false;
    }
    FR_TRY(join_side(m, s));   // anchor nets of frcnn_pnet_forward_async_heads still in flight (image without examples)
    if (backbone_trained(m)) FR_TRY(fill_zero((char*)m->zero_arena.p + m->delta_bytes, m->gpool_bytes, s));
    FR_TRY(backward_heads(m, w, grad, s, 0));
  }
  return FRCNN_OK;
}

// What the weight-gradient launch of convolution (b, st) takes besides its output gradient
struct WgradArgs {
  const float* in; const float* in_slope = nullptr; const float* in_scale = nullptr;   // the input tensor, its pending PReLU / SpatialDropout
  int cin, o;                                             // channels / filters of the launch
  WgradMap map; bool mapped = false;                      // compact block: where the gathered channels / filters belong
  const float* wa_in = nullptr; const float* wa_g = nullptr;   // fp16 form: magnitude records of the input / the output gradient
};
static WgradArgs wgrad_args(const frcnn_model* m, const float* w, int b, int st) {
  const Block& blk = m->blocks[b];
  const Conv& c = m->convs[blk.first_conv + st];
  WgradArgs a;
  // accGradParameters: the input is the previous conv's x (activation fused) or a pooled map / image
  if (st > 0) {
    const Conv& pc = m->convs[blk.first_conv + st - 1];
    a.in = pc.x.f(); a.in_slope = w + pc.a_off;
    a.in_scale = (st - 1 == 0 && blk.has_drop) ? blk.scale.f() : nullptr;
  } else {
    a.in = b == 0 ? m->img.f() : m->blocks[b - 1].pooled.f();
  }
  // compact block (Block::dc_on): the second convolution's weight gradient is computed for the kept input channels (its
  // input IS the compact tensor; their dropout scale is 1), the first one's for the kept filters (its output gradient is
  // compact); the fold scatters both into the full tensors, the bias gradient follows the filter map
  a.cin = c.Cin; a.o = c.Cout;
  a.mapped = blk.dc_on && st <= 1;
  if (a.mapped) {
    a.map.Cfull = c.Cin;
    if (st == 1) { a.cin = blk.nkM; a.map.cmap = blk.dc_idx; a.in_scale = nullptr; }
    else { a.o = blk.nkM; a.map.omap = blk.dc_idx; }
  }
  // fp16 form of the weight-gradient launch: the records of both tensors exist when the forward launch that wrote `in` and
  // the backward launch that wrote c.gx kept them (the same two tensors feed c's forward and c's input gradient)
  if (m->f16_packed && c.x_f && c.x_d && (st > 0 || b > 0)) {
    a.wa_in = st > 0 ? m->rec(m->convs[blk.first_conv + st - 1].am) : m->rec(m->blocks[b - 1].am);
    a.wa_g = m->rec(c.am + 1);
  }
  return a;
}

int frcnn_pnet_backward(frcnn_model* m, const float* w, float* grad, void* stream) {
  hipStream_t s = S(stream);
  FR_CHECK(m->H > 0 && m->training, "pnet_backward: needs a preceding training-mode forward "
                                    "(nn.SpatialDropout: backprop only defined while training)");
  const int nb = (int)m->blocks.size();
  for (auto& c : m->convs) m->am_live[c.am + 1] = 0;
  bool heads_tail = false;   // anchor nets still computing their parameter gradients on their own streams: joined at the end
  FR_TRY(join_anchor_nets_for_backbone(m, w, grad, s, &heads_tail));
  // staged training (frcnn_model_set_trainable): blocks 0..fb-1 are frozen; the chain stops at block fb, whose first convolution
  // computes its weight gradient and no input gradient
  const int fb = m->frozen_blocks;
  if (fb < nb) {  // output nheads+1 is the last pooled map itself (model_utilities.lua:55)
    // (nobody has zeroed the pooled maps' gradients when the anchor nets are frozen: the chain below adds into them)
    if (!m->train_heads) FR_TRY(fill_zero((char*)m->zero_arena.p + m->delta_bytes, m->gpool_bytes, s));
    Block& last = m->blocks.back();
    FR_TRY(add_inplace(last.gpooled.f(), m->delta_last.f(), (long)m->d.filters[nb - 1] * last.Hp * last.Wp, s));
  }
  // from here on the caller's stream is busy with matrix-core work for the rest of the pass (frcnn_pnet_wait_backward_begun)
  if (m->update_armed) FR_TRY(m->bwd_ev.record(s));
  // a frozen block's gradients are final and its weights free at once: its events mark this point of the caller's stream
  for (int b = 0; b < fb; ++b) FR_TRY(mark_block_done(m, b, s));
  // The weight gradient of a layer and the input gradient that feeds the next act_backward are independent:
  // accGradParameters goes to a side stream, so its blocks fill the CUs that the tail of the updateGradInput
  // kernel (one wave of blocks, retiring unevenly) leaves idle, and the ~4 us dispatch gaps of one chain
  // are covered by the other.
  const bool use_side = side_enabled();
  if (use_side) FR_TRY(ensure_side(m));
  hipStream_t ws = use_side ? m->side : s;
  size_t n_fork = 0;
  // Fused activation backward (round 4): the input-gradient launch of convolution st writes its result THROUGH the backward of
  // convolution st - 1's PReLU / SpatialDropout (conv_x3's X3PostAct: epilogue, or the fold of its split-K slabs) and adds the
  // slope gradient; the bias gradient of st - 1 rides on its weight-gradient launch (conv_wgrad's gbias).  act_backward --
  // a read-read-write pass over the tensor on the dependent chain -- is then not launched for st - 1.  (Not in deterministic
  // mode: the sums leave through atomics.)
  const bool fuse_act = fuse_act_on();
  bool act_done = false;   // the gradient tensor of the convolution being visited already went through its activation
  for (int b = nb - 1; b >= fb; --b) {
    Block& blk = m->blocks[b];
    for (int st = blk.nconv - 1; st >= 0; --st) {
      Conv& c = m->convs[blk.first_conv + st];
      const float* scale = (st == 0 && blk.has_drop) ? blk.scale.f() : nullptr;
      const bool fused_here = act_done;
      act_done = false;
      // the very first convolution when it is its block's only one: its input gradient is not needed, so the pooling + PReLU
      // backward is computed inside its weight-gradient launch and the full-resolution gradient never exists
      static const bool first_pooled_on = env_flag("FRCNN_FIRST_POOLED", true);
      const bool first_pooled = fuse_act && first_pooled_on && b == 0 && st == 0 && blk.nconv == 1 && scale == nullptr &&
                                conv_wgrad_first_pooled_eligible(c.Cin, c.Cout, c.k, c.Wo);
      if (first_pooled) {
        // (on the caller's stream with the slab workspace of its own, like the unfused first layer: see on_caller below)
        FR_TRY(conv_wgrad_first_pooled(m->img.f(), c.Cin, c.H, c.W, blk.gpooled.f(), (const unsigned char*)blk.pidx.p, c.x.f(),
                                       w + c.a_off, c.Cout, c.pad, grad + c.w_off, grad + c.b_off, grad + c.a_off,
                                       m->wg_ws_first.p, m->wg_ws_first.bytes, s));
        FR_TRY(mark_block_done(m, b, s));
        break;
      }
      if (fused_here) {
        // (nothing: c.gx is final; its bias gradient comes with the weight gradient below)
      } else if (st == blk.nconv - 1) {
        FR_TRY(maxpool_act_backward(blk.gpooled.f(), (const unsigned char*)blk.pidx.p, c.x.f(), c.Cout, c.Ho, c.Wo,
                                    w + c.a_off, scale, c.gx.f(), grad + c.b_off, grad + c.a_off, s,
                                    (c.x_d && m->f16_packed) ? m->rec_w(c.am + 1) : nullptr));
      } else {
        FR_TRY(act_backward(c.gx.f(), c.x.f(), c.Cout, (long)c.Ho * c.Wo, w + c.a_off, scale, c.gx.f(),
                            grad + c.b_off, grad + c.a_off, s, (c.x_d && m->f16_packed) ? m->rec_w(c.am + 1) : nullptr));
      }
      const WgradArgs wa = wgrad_args(m, w, b, st);
      const bool dc = wa.mapped;
      // The first layer's weight gradient ends the pass and the caller's stream has nothing left to do (no input gradient for
      // the image): it runs THERE, with a slab workspace of its own, beside the side stream's last launches instead of
      // behind them (the optimiser waited ~80 us for the side stream's tail).
      const bool on_caller = use_side && b == 0 && st == 0;
      if (use_side && !on_caller) FR_TRY(fork_side(m, s, n_fork++));   // c.gx is final here
      const hipStream_t wgs = on_caller ? s : ws;
      const DevBuf& slabs = on_caller ? m->wg_ws_first : m->wg_ws;
      FR_TRY(conv_wgrad(wa.in, wa.cin, c.H, c.W, wa.in_slope, wa.in_scale, c.gx.f(), wa.o, c.k, c.pad, grad + c.w_off, slabs.p, slabs.bytes, wgs,
                        fused_here ? grad + c.b_off : nullptr, wa.wa_in, wa.wa_g, dc ? &wa.map : nullptr));
      if (on_caller) FR_TRY(join_side_now(m, s));   // (block 0's other convolutions, if any, are on the side stream)
      // every gradient of block b's parameters is final once this launch has run (its fork also covers the bias / slope sums
      // that act_backward accumulates on the caller's stream)
      if (st == 0) FR_TRY(m->block_ev[b].record(wgs));
      if (b == fb && st == 0) {   // gradInput of the first conv is unused (objective.lua:189), so is a frozen block's
        FR_TRY(record_block_read(m, b, s));
        break;
      }
      float* gin = st > 0 ? m->convs[blk.first_conv + st - 1].gx.f() : m->blocks[b - 1].gpooled.f();
      const int gmode = st > 0 ? OUT_STORE : OUT_ADD;
      // fp16 form: the magnitude of c.gx was recorded by the launch that finished it (the pooling / activation backward above,
      // or the previous input-gradient launch through its fused activation backward)
      const float* ag = nullptr;
      const float* aw = nullptr;
      if (c.x_d && m->f16_packed) { ag = m->rec(c.am + 1); aw = m->amax_ws.f() + c.am; }
      // compact block: the second convolution's input gradient is computed for the kept channels only and stored compact (it
      // passes through the first convolution's PReLU; the kept channels' dropout scale is 1); the first convolution's reads
      // that compact gradient: K = the kept filters
      const int dg_k = (dc && st == 0) ? blk.nkK : c.Cout, dg_m = (dc && st == 1) ? blk.nkM : c.Cin;
      const double fl = 2.0 * dg_k * dg_m * c.k * c.k * (double)c.Ho * c.Wo;
      if (c.x_d && st > 0 && fuse_act && c.k == 3) {
        Conv& pc = m->convs[blk.first_conv + st - 1];
        X3PostAct post{pc.x.f(), w + pc.a_off, (st - 1 == 0 && blk.has_drop && !dc) ? blk.scale.f() : nullptr, grad + pc.a_off};
        FR_TRY(conv_x3(c.gx.f(), dg_k, c.Ho, c.Wo, nullptr, nullptr, c.wxd.p, nullptr, dg_m, c.k, c.k - 1 - c.pad, gin, gmode, fl, s, 0, &post, ag, aw,
                       (pc.x_d && m->f16_packed) ? m->rec_w(pc.am + 1) : nullptr));
        act_done = true;
      } else if (c.x_d)
        FR_TRY(conv_x3(c.gx.f(), dg_k, c.Ho, c.Wo, nullptr, nullptr, c.wxd.p, nullptr, dg_m, c.k, c.k - 1 - c.pad, gin, gmode, fl, s, 0, nullptr, ag, aw));
      else
        FR_TRY(conv_igemm(c.gx.f(), c.Cout, c.Ho, c.Wo, nullptr, nullptr, c.wd.f(), nullptr, c.Cin, c.k,
                          c.k - 1 - c.pad, gin, gmode, fl, s));
      if (st == 0) FR_TRY(record_block_read(m, b, s));   // the block's weights, packs and weight magnitudes have had their last reader
    }
  }
  m->block_ev_valid = true;
  if (heads_tail && !m->heads_gin) FR_TRY(join_heads(m, s));   // the anchor nets' parameter gradients (see above; the sparse path's are on the side stream, joined below)
  FR_TRY(cw_join(m, s));   // the classification net's weight gradients (frcnn_cnet_backward) belong to the same gradient vector
  if (use_side) {   // the caller's stream continues after every weight gradient has landed
    FR_TRY(join_side_now(m, s));
    m->side_busy = false;
  }
  return FRCNN_OK;
}

// ------------------------------------------------------------------------------------ cnet
// the row-wise layers fused with the folds of the products around them (cnet.hip: "fused forms"); FRCNN_CNET_FUSE=0: one launch each
static bool cnet_fuse() { return env_flag("FRCNN_CNET_FUSE", true); }   // (read per call: the tests switch it)
static int ensure_cnet(frcnn_model* m, int R) {
  for (auto& L : m->cls) {
    size_t n = (size_t)R * L.n * 4;
    FR_TRY(L.lin.ensure(n));
    if (L.bn) { FR_TRY(L.pre.ensure(n)); FR_TRY(L.xhat.ensure(n)); FR_TRY(L.invstd.ensure((size_t)L.n * 4)); }
    FR_TRY(L.post.ensure(n));
    FR_TRY(L.g.ensure(n));
    FR_TRY(L.gin.ensure((size_t)R * L.in * 4));
    if (L.p_drop > 0.f) FR_TRY(L.mask.ensure(n));
    FR_TRY(L.fc.ensure(R, L.in, L.n, 7));
  }
  int nc = m->d.class_count + 1;
  int nf = m->cls.empty() ? m->D : m->cls.back().n;
  FR_TRY(m->feat_g.ensure((size_t)R * nf * 4));
  FR_TRY(m->logits.ensure((size_t)R * nc * 4));
  FR_TRY(m->lsm.ensure((size_t)R * nc * 4));
  FR_TRY(m->glog.ensure((size_t)R * nc * 4));
  if (m->d.box_per_class) FR_TRY(m->box_sel.ensure((size_t)R * 4));
  return FRCNN_OK;
}

int frcnn_cnet_box_classes(frcnn_model* m, const void* classes, int kind, int n) {
  FR_CHECK(m != nullptr, "cnet_box_classes: null model");
  FR_CHECK(m->d.box_per_class, "cnet_box_classes: the model's box head is shared (frcnn_model_desc.box_per_class is 0)");
  FR_CHECK(kind >= 0 && kind <= 2, "cnet_box_classes: class source %d (0 none, 1 int32, 2 fp32)", kind);
  FR_CHECK(kind == 0 || classes, "cnet_box_classes: class source %d without classes", kind);
  FR_CHECK(kind != 1 || n >= 0, "cnet_box_classes: %d foreground rows", n);
  m->box_classes = kind ? classes : nullptr; m->box_kind = kind; m->box_n = kind == 1 ? n : 0;
  return FRCNN_OK;
}

int frcnn_cnet_forward(frcnn_model* m, const float* weights, const float* x, int R, int training,
                       const float* const* drop_masks, unsigned long long seed, float* bn_running,
                       float* bbox_out, float* cls_out, void* stream) {
  hipStream_t s = S(stream);
  // the class source of the per-class box head serves this call only, whatever becomes of it
  const void* box_classes = m->box_classes;
  const int box_kind = m->box_kind, box_n = m->box_n;
  m->box_classes = nullptr; m->box_kind = 0; m->box_n = 0;
  FR_CHECK(R > 0, "cnet_forward: empty batch");
  FR_CHECK(box_kind != 1 || box_n <= R, "cnet_forward: %d foreground classes for %d rows (frcnn_cnet_box_classes)", box_n, R);
  FR_TRY(cw_join(m, s));   // (weight gradients of a previous backward pass still read the buffers written below)
  FR_TRY(ensure_cnet(m, R));
  m->R = R; m->cnet_x = x; m->training = training;
  const float* w = weights;
  const float* cur = x;
  float* bnr = bn_running;
  for (size_t l = 0; l < m->cls.size(); ++l) {
    ClsLayer& L = m->cls[l];
    GemmFold fold;   // (fused: the layer's row-wise kernel folds the product's split-K slabs itself)
    GemmFold* defer = cnet_fuse() ? &fold : nullptr;
    // (evaluate mode under static_weights: the weight matrix's magnitude record is kept within one generation)
    FR_TRY(L.fc.forward(cur, w + L.w_off, w + L.b_off, L.lin.f(), (!training && g_static_weights) ? g_static_gen : -1, s, 0, defer));
    if (L.bn) FR_CHECK(training || bnr, "cnet_forward: evaluate mode needs bn_running");
    const float* mask = nullptr;
    float inv_keep = 1.f;
    bool draw = false;
    if (training && L.p_drop > 0.f) {  // nn.Dropout v2: train = mask/(1-p), evaluate = identity [ext]
      inv_keep = 1.0f / (1.0f - L.p_drop);
      if (drop_masks && drop_masks[l])
        FR_HIP(hipMemcpyAsync(L.mask.p, drop_masks[l], (size_t)R * L.n * 4, hipMemcpyDeviceToDevice, s));
      else
        draw = true;   // mask drawn inside the activation kernel
      mask = L.mask.f();
    }
    if (defer) {   // fold -> [BatchNormalization ->] PReLU -> Dropout: one launch
      FR_TRY(cnet_act_forward(L.lin.f(), fold, R, L.n, L.bn ? w + L.bnw_off : nullptr, L.bn ? w + L.bnb_off : nullptr, L.bn ? bnr : nullptr,
                              training, L.lin.f(), L.xhat.f(), L.invstd.f(), L.pre.f(), w + L.a_off, const_cast<float*>(mask), draw,
                              inv_keep, L.p_drop, seed * 977 + l + 17, L.post.f(), s));
      if (L.bn && bnr) bnr += 2 * L.n;
      cur = L.post.f();
      continue;
    }
    const float* pre = L.lin.f();
    if (L.bn) {
      FR_TRY(bn_forward(L.lin.f(), R, L.n, w + L.bnw_off, w + L.bnb_off, bnr, training, L.xhat.f(), L.invstd.f(),
                        L.pre.f(), s));
      if (bnr) bnr += 2 * L.n;
      pre = L.pre.f();
    }
    if (draw)
      FR_TRY(prelu_dropout_forward_gen(pre, (long)R * L.n, w + L.a_off, L.mask.f(), L.p_drop, seed * 977 + l + 17,
                                       L.post.f(), s));
    else
      FR_TRY(prelu_dropout_forward(pre, (long)R * L.n, w + L.a_off, mask, inv_keep, L.post.f(), s));
    cur = L.post.f();
  }
  const int nf = m->cls.empty() ? m->D : m->cls.back().n;
  const int nc = m->d.class_count + 1;
  if (m->d.box_per_class) {
    // the class head first: without a class source a row's box is the one of the class its own log-probabilities predict
    if (cnet_fuse()) {
      GemmFold fold;
      FR_TRY(gemm_f32(cur, nf, 1, w + m->clsw_off, 1, nf, m->logits.f(), nc, R, nc, nf, OUT_STORE, w + m->clsb_off, s, 0, &fold));
      FR_TRY(log_softmax_rows_fold(m->logits.f(), fold, R, nc, m->lsm.f(), cls_out, s));
    } else {
      FR_TRY(gemm_f32(cur, nf, 1, w + m->clsw_off, 1, nf, m->logits.f(), nc, R, nc, nf, OUT_STORE, w + m->clsb_off, s));
      FR_TRY(log_softmax_rows(m->logits.f(), R, nc, m->lsm.f(), s));
      FR_HIP(hipMemcpyAsync(cls_out, m->lsm.p, (size_t)R * nc * 4, hipMemcpyDeviceToDevice, s));
    }
    return box_head_forward(cur, R, nf, w + m->bbox_w_off, w + m->bbox_b_off, m->d.class_count, box_classes, box_kind, box_n,
                            m->lsm.f(), nc, bbox_out, (int*)m->box_sel.p, s);
  }
  if (cnet_fuse() && cnet_heads_fused_eligible(nf, nc)) {   // both heads, nn.LogSoftMax and the copy to the caller's tensor: one launch
    return cnet_heads_forward(cur, R, nf, w + m->bbox_w_off, w + m->bbox_b_off, w + m->clsw_off, w + m->clsb_off, nc, bbox_out,
                              m->logits.f(), m->lsm.f(), cls_out, s);
  }
  FR_TRY(gemm_f32(cur, nf, 1, w + m->bbox_w_off, 1, nf, bbox_out, 4, R, 4, nf, OUT_STORE, w + m->bbox_b_off, s));
  if (cnet_fuse()) {   // the class head's fold, nn.LogSoftMax and the copy to the caller's tensor: one launch
    GemmFold fold;
    FR_TRY(gemm_f32(cur, nf, 1, w + m->clsw_off, 1, nf, m->logits.f(), nc, R, nc, nf, OUT_STORE, w + m->clsb_off, s, 0, &fold));
    FR_TRY(log_softmax_rows_fold(m->logits.f(), fold, R, nc, m->lsm.f(), cls_out, s));
    return FRCNN_OK;
  }
  FR_TRY(gemm_f32(cur, nf, 1, w + m->clsw_off, 1, nf, m->logits.f(), nc, R, nc, nf, OUT_STORE, w + m->clsb_off, s));
  FR_TRY(log_softmax_rows(m->logits.f(), R, nc, m->lsm.f(), s));
  FR_HIP(hipMemcpyAsync(cls_out, m->lsm.p, (size_t)R * nc * 4, hipMemcpyDeviceToDevice, s));
  return FRCNN_OK;
}

// the box head's input of the last forward pass (R x nf: the last class layer's output, or the caller's input without class
// layers) -> dst, on `stream`
int frcnn_cnet_features(frcnn_model* m, float* dst, void* stream) {
  FR_CHECK(m != nullptr, "cnet_features: null model");
  FR_CHECK(m->R > 0, "cnet_features: call frcnn_cnet_forward first");
  FR_CHECK(dst != nullptr, "cnet_features: NULL dst");
  const int nf = m->cls.empty() ? m->D : m->cls.back().n;
  const float* feat = m->cls.empty() ? m->cnet_x : m->cls.back().post.f();
  FR_HIP(hipMemcpyAsync(dst, feat, (size_t)m->R * nf * 4, hipMemcpyDeviceToDevice, S(stream)));
  return FRCNN_OK;
}

int frcnn_cnet_backward(frcnn_model* m, const float* weights, const float* g_bbox, const float* g_cls, float* gx,
                        float* grad, void* stream) {
  hipStream_t s = S(stream);
  FR_CHECK(m->R > 0, "cnet_backward: call frcnn_cnet_forward first");
  const int R = m->R;
  const float* w = weights;
  const int nf = m->cls.empty() ? m->D : m->cls.back().n;
  const int nc = m->d.class_count + 1;
  const float* feat = m->cls.empty() ? m->cnet_x : m->cls.back().post.f();
  // staged training with the whole backbone frozen: nobody reads the input gradient -- the chain's last product (and its magnitude
  // and split passes) is not queued, gx stays unwritten
  if (m->frozen_blocks >= (int)m->blocks.size()) gx = nullptr;
  // `s` carries the input-gradient chain (what roi_pool_backward and the backbone wait for); the weight-gradient products and
  // bias sums go to `ws`: a stream of their own (see g_cnet_wgrad_async), or `s` itself
  FR_TRY(cw_join(m, s));
  const bool async = g_cnet_wgrad_async && !deterministic();
  if (async) FR_TRY(ensure_update_stream(m));
  hipStream_t ws = async ? m->cw : s;
  const int wslot = async ? 7 : 0;     // split-K workspace of the products on `ws`
  size_t nfork = 0;
  auto fork = [&]() -> int {           // everything queued on `s` so far is final for `ws`
    return async ? chain(s, ws, m->cw_ev[nfork++]) : FRCNN_OK;
  };
  // heads: LogSoftMax backward first, then the two input gradients on the chain, the two weight gradients beside it
  bool top_act_done = false;   // the last hidden layer's Dropout + PReLU backward was applied by the heads' launch (L.g is final)
  const bool per_class = m->d.box_per_class != 0;   // (the fused two-heads launches know the shared box head only)
  if (!per_class && cnet_fuse() && cnet_heads_fused_eligible(nf, nc)) {   // LogSoftMax backward + both input gradients: one launch
    HeadsPostAct post;
    float* dst = m->feat_g.f();
    if (!m->cls.empty() && !m->cls.back().bn && !deterministic()) {
      ClsLayer& T = m->cls.back();
      const bool drop = m->training && T.p_drop > 0.f;
      post.pre = T.lin.f(); post.mask = drop ? T.mask.f() : nullptr; post.inv_keep = drop ? 1.0f / (1.0f - T.p_drop) : 1.f;
      post.slope = w + T.a_off; post.gslope = grad + T.a_off;
      dst = T.g.f();
      top_act_done = true;
    }
    FR_TRY(cnet_heads_backward(g_bbox, g_cls, m->lsm.f(), R, nf, w + m->bbox_w_off, w + m->clsw_off, nc, m->glog.f(), dst, s,
                               top_act_done ? &post : nullptr));
    FR_TRY(fork());
  } else {
    FR_TRY(log_softmax_backward(g_cls, m->lsm.f(), R, nc, m->glog.f(), s));
    FR_TRY(fork());
    if (per_class)   // the rows of each example's class, stored; the class head's input gradient is added on top
      FR_TRY(box_head_backward(g_bbox, nullptr, (const int*)m->box_sel.p, R, nf, w + m->bbox_w_off, m->d.class_count, m->feat_g.f(),
                               nullptr, nullptr, s, s));
    else
      FR_TRY(gemm_f32(g_bbox, 4, 1, w + m->bbox_w_off, nf, 1, m->feat_g.f(), nf, R, nf, 4, OUT_STORE, nullptr, s));
    FR_TRY(gemm_f32(m->glog.f(), nc, 1, w + m->clsw_off, nf, 1, m->feat_g.f(), nf, R, nf, nc, OUT_ADD, nullptr, s));
  }
  if (per_class) {   // the box head's weight and bias gradient, segmented by class (classes without a row are not touched)
    FR_TRY(box_head_backward(g_bbox, feat, (const int*)m->box_sel.p, R, nf, nullptr, m->d.class_count, nullptr, grad + m->bbox_w_off,
                             grad + m->bbox_b_off, ws, ws));
  } else {
    FR_TRY(gemm_f32(g_bbox, 1, 4, feat, nf, 1, grad + m->bbox_w_off, nf, 4, nf, R, OUT_ADD, nullptr, ws, wslot));
    FR_TRY(channel_sum_cols(g_bbox, R, 4, grad + m->bbox_b_off, ws));
  }
  FR_TRY(gemm_f32(m->glog.f(), 1, nc, feat, nf, 1, grad + m->clsw_off, nf, nc, nf, R, OUT_ADD, nullptr, ws, wslot));
  FR_TRY(channel_sum_cols(m->glog.f(), R, nc, grad + m->clsb_off, ws));
  const float* g = m->feat_g.f();
  GemmFold gfold;   // (fused: the gradient arriving from the layer above is a product whose slabs this layer's kernel folds)
  for (int l = (int)m->cls.size() - 1; l >= 0; --l) {
    ClsLayer& L = m->cls[l];
    const float* pre = L.bn ? L.pre.f() : L.lin.f();
    const bool drop = m->training && L.p_drop > 0.f;
    if (top_act_done && l == (int)m->cls.size() - 1) {
      // (nothing: the heads' launch stored L.g)
    } else if (L.bn && cnet_fuse()) {   // Dropout -> PReLU -> BatchNormalization backward: one launch
      FR_TRY(cnet_act_bn_backward(g, gfold, pre, L.xhat.f(), L.invstd.f(), w + L.bnw_off, w + L.a_off, drop ? L.mask.f() : nullptr,
                                  drop ? 1.0f / (1.0f - L.p_drop) : 1.f, R, L.n, m->training, L.g.f(), grad + L.bnw_off,
                                  grad + L.bnb_off, grad + L.a_off, s));
    } else {
      FR_TRY(prelu_dropout_backward(g, pre, (long)R * L.n, w + L.a_off, drop ? L.mask.f() : nullptr,
                                    drop ? 1.0f / (1.0f - L.p_drop) : 1.f, L.g.f(), grad + L.a_off, s));
      if (L.bn)
        FR_TRY(bn_backward(L.g.f(), L.xhat.f(), L.invstd.f(), w + L.bnw_off, R, L.n, m->training, L.g.f(),
                           grad + L.bnw_off, grad + L.bnb_off, s));
    }
    gfold = GemmFold{};
    // the input gradient of this layer is folded by the layer below when that one runs the fused kernel and nothing else
    // touches this stream's split-K workspace in between (the weight-gradient products are on their own stream and slot)
    GemmFold* gdefer = (cnet_fuse() && async && l > 0 && m->cls[l - 1].bn) ? &gfold : nullptr;
    FR_TRY(fork());   // L.g is final
    const float* in = l == 0 ? m->cnet_x : m->cls[l - 1].post.f();
    float* gin = l == 0 ? gx : L.gin.f();
    // chain: the input-gradient product; beside it: the weight gradient and the bias sums
    FR_TRY(L.fc.dgrad(L.g.f(), w + L.w_off, gin, s, 0, gdefer));
    FR_TRY(L.fc.wgrad(L.g.f(), in, w + L.w_off, grad + L.w_off, grad + L.b_off, ws, wslot));
    g = gin;
  }
  if (m->cls.empty() && gx) FR_HIP(hipMemcpyAsync(gx, g, (size_t)R * m->D * 4, hipMemcpyDeviceToDevice, s));
  if (async) {
    FR_TRY(m->cw_done.record(ws));
    m->cw_pending = true;
  }
  return FRCNN_OK;
}

}  // extern "C"
