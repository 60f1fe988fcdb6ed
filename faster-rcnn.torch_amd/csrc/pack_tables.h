// pack_tables.h -- the device job tables of the weight packs: which weight tensor of the proposal net gets which pack job, and the
// named parts of the tables that the passes of net.cpp launch from.  Host bookkeeping only.  Included behind common.h, kernels.h
// and own.h: it uses their declarations and makes none itself (tests/pack_tables_host_check.cpp compiles it against stand-ins).
// Three job kinds, one table each: PackJob (fp32 packs), AmaxJob (the weight tensors' magnitude records of the fp16 split form)
// and PackXJob (split-operand packs; every list twice: plain, and with the weight tensor's magnitude attached for the fp16 form).
// A table is a row of lists; each list had its blocks assigned on its own and is launched on its own, through the Span naming it.
// Packs by owner: group b < nblocks = backbone block b, group nblocks = the anchor nets.  Each group has lists of its own, so that
// frcnn_pnet_refresh_packs can renew one owner's packs as soon as ITS slice of the weight vector has been updated; a training
// forward whose groups are all fresh for the weight vector it is given skips the model-wide launches.
#pragma once
#include <vector>

namespace frcnn {

struct Span { int off = 0, n = 0, grid = 0; };   // jobs [off, off + n) of a table and the grid that runs them; empty: grid 0

template <class Job>
struct JobTable {
  std::vector<Job> host;
  DevBuf dev;
  // assigns blocks on `list` alone (assign(jobs, n) -> grid; not called for an empty list), appends it and names it
  template <class Assign>
  Span append(std::vector<Job> list, Assign assign) {
    Span sp;
    sp.off = (int)host.size(); sp.n = (int)list.size();
    if (sp.n) sp.grid = assign(list.data(), sp.n);
    host.insert(host.end(), list.begin(), list.end());
    return sp;
  }
  int upload() {   // (blocking: the host vector may change behind it)
    if (host.empty()) return FRCNN_OK;
    FR_TRY(dev.ensure(host.size() * sizeof(Job)));
    FR_HIP(hipMemcpy(dev.p, host.data(), host.size() * sizeof(Job), hipMemcpyHostToDevice));
    return FRCNN_OK;
  }
  const Job* at(const Span& sp) const { return (const Job*)dev.p + sp.off; }   // device jobs of a span
  const Job* host_at(const Span& sp) const { return host.data() + sp.off; }    // ... their host copies
};

// One weight tensor of the proposal net and what the rules below need to know of it.
struct PackTensor {
  enum Kind { BACKBONE, HEAD_C3, HEAD_C1 } kind = BACKBONE;   // a backbone convolution | an anchor net's k x k | its 1 x 1 convolution
  int group = 0, conv = -1; // owner; index into the backbone's convolutions (-1: an anchor net's)
  bool first = false;       // the network's first convolution: no input gradient
  bool x_f = false, x_d = false;   // the forward / input-gradient launch takes the split form
  int am = -1;              // first of the tensor's magnitude records (am + 2: the weights')
  long w_off = 0;
  int Cout = 0, Cin = 0, k = 0, H = 0, W = 0, Ho = 0, Wo = 0;
  float *wf = nullptr, *wd = nullptr;    // fp32 packs (forward / input gradient)
  void *wx = nullptr, *wxd = nullptr;    // split-operand packs

  bool head() const { return kind != BACKBONE; }
  // mode 0 forward, 1 input gradient.  The 1 x 1 convolutions never take the split form.
  bool split(int mode) const { return kind != HEAD_C1 && (mode ? x_d : x_f); }
  // the fp32 pack of the launches that do not.  An anchor net's input-gradient packs are needed by the dense backward only
  // (PackTables::pk_heads, renewed lazily) and belong to no other list.
  bool fp32(int mode) const { return mode == 0 ? !split(0) : head() || (!first && !x_d); }
  bool has_record() const { return split(0) || split(1); }   // its weights' magnitude is taken (fp16 form)
};

struct PackTables {
  JobTable<PackJob> pack;
  JobTable<AmaxJob> amax;
  JobTable<PackXJob> x3;
  std::vector<PackTensor> tensors;   // backbone convolutions in order, then each anchor net's c3 and c1
  // PackJob lists: a training pass (forward jobs, then the backbone's input-gradient jobs) | an evaluate-mode pass | the anchor
  // nets' input-gradient packs | the backbone's training packs (a pass that runs the anchor nets sparse)
  Span pk_train, pk_fwd, pk_heads, pk_bb;
  Span am_all, am_bb;                // AmaxJob lists: every split tensor | the backbone's
  Span x3_train[2], x3_fwd[2];       // PackXJob lists, [0] plain | [1] fp16 form: a training pass | an evaluate-mode pass
  struct Group { Span pk, am, x3[2]; };
  std::vector<Group> groups;         // training packs by owner
  std::vector<int> x3_conv;          // job i of x3_train belongs to this backbone convolution (-1: an anchor net); pack_compact
                                     // re-writes the jobs of x3.host_at(x3_train[f16]) step by step

  bool f16() const { return get_x3_f16() && am_all.n > 0; }   // the split launches run in the fp16 form

  template <class Job> struct Tagged { Job job; int t, mode; };   // a job of tensors[t]
  template <class Job, class Pred>
  std::vector<Job> pick(const std::vector<Tagged<Job>>& from, Pred pred) const {
    std::vector<Job> r;
    for (auto& e : from) if (pred(tensors[e.t], e.mode)) r.push_back(e.job);
    return r;
  }

  // rec0 / ws0: the model's magnitude records and weight-magnitude scalars.  Uploads nothing: see upload().
  int build(std::vector<PackTensor> ts, int nblocks, float* rec0, float* ws0) {
    tensors = std::move(ts);
    pack.host.clear(); amax.host.clear(); x3.host.clear(); x3_conv.clear();
    // every job of every tensor, in the order of `tensors`, a tensor's forward job before its input-gradient job: the one place
    // that constructs jobs.  Every list below is a selection from these.
    std::vector<Tagged<PackJob>> pk;
    std::vector<Tagged<AmaxJob>> am;
    std::vector<Tagged<PackXJob>> xs[2];
    for (int i = 0; i < (int)tensors.size(); ++i) {
      const PackTensor& t = tensors[i];
      float* rec_w = t.has_record() ? rec0 + (size_t)(t.am + 2) * AMAX_REC : nullptr;
      for (int mode : {0, 1}) {
        if (t.fp32(mode)) pk.push_back({conv_pack_job(t.w_off, t.Cout, t.Cin, t.k, mode, mode ? t.wd : t.wf), i, mode});
        if (!t.split(mode)) continue;
        // (built for the output map of the launch it feeds)
        PackXJob j = mode ? conv_x3_pack_job(t.w_off, t.Cout, t.Cin, t.k, 1, t.wxd, t.H, t.W)
                          : conv_x3_pack_job(t.w_off, t.Cout, t.Cin, t.k, 0, t.wx, t.Ho, t.Wo);
        xs[0].push_back({j, i, mode});
        j.amax = rec_w; j.amax_w = ws0 + t.am;
        xs[1].push_back({j, i, mode});
        x3_conv.push_back(t.conv);
      }
      if (t.has_record()) am.push_back({AmaxJob{t.w_off, (long)t.Cout * t.Cin * t.k * t.k, rec_w, 0}, i, 0});
    }
    auto any = [](const PackTensor&, int) { return true; };
    auto fwd = [](const PackTensor&, int mode) { return mode == 0; };
    auto backbone = [](const PackTensor& t, int) { return !t.head(); };
    auto heads_dgrad = [](const PackTensor& t, int mode) { return t.head() && mode == 1; };
    auto add_pk = [&](std::vector<PackJob> list, int budget) {
      return pack.append(std::move(list), [budget](PackJob* j, int n) { return conv_pack_assign_blocks(j, n, budget); });
    };
    auto add_am = [&](std::vector<AmaxJob> list, Span* sp) -> int {
      *sp = amax.append(std::move(list), tensor_absmax_assign_blocks);
      FR_CHECK(sp->grid >= 0, "ensure_shapes: a weight tensor is too large for its magnitude record");
      return FRCNN_OK;
    };
    groups.assign((size_t)nblocks + 1, Group());
    std::vector<PackJob> train = pick(pk, fwd);
    for (auto& j : pick(pk, [](const PackTensor& t, int mode) { return !t.head() && mode == 1; })) train.push_back(j);
    pk_train = add_pk(std::move(train), 2048);
    pk_fwd = add_pk(pick(pk, fwd), 2048);
    pk_heads = add_pk(pick(pk, heads_dgrad), 2048);
    pk_bb = add_pk(pick(pk, backbone), 512);
    FR_TRY(add_am(pick(am, any), &am_all));
    FR_TRY(add_am(pick(am, backbone), &am_bb));
    for (int f = 0; f < 2; ++f) {
      x3_train[f] = x3.append(pick(xs[f], any), conv_x3_pack_assign_blocks);
      x3_fwd[f] = x3.append(pick(xs[f], fwd), conv_x3_pack_assign_blocks);
    }
    for (int g = 0; g <= nblocks; ++g) {
      auto mine = [g](const PackTensor& t, int) { return t.group == g; };
      groups[g].pk = add_pk(pick(pk, [&](const PackTensor& t, int mode) { return t.group == g && !heads_dgrad(t, mode); }), 512);
      FR_TRY(add_am(pick(am, mine), &groups[g].am));
      for (int f = 0; f < 2; ++f) groups[g].x3[f] = x3.append(pick(xs[f], mine), conv_x3_pack_assign_blocks);
    }
    return FRCNN_OK;
  }

  int upload() { FR_TRY(pack.upload()); FR_TRY(amax.upload()); return x3.upload(); }
};

}  // namespace frcnn
