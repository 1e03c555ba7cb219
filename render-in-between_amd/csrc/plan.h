// plan.h — the data model of a launch plan: what the builder (planner.h) writes and run_plan (rib.hip) reads.
// A part of rib.hip's translation unit, included there once, behind the kernel parameter structs and the variant table.
#pragma once

namespace {

enum OpKind { OP_PACK, OP_IGEMM, OP_FINALIZE, OP_POOL, OP_INADD, OP_SPLITEPI, OP_MODULATE, OP_WINO_IN, OP_WINO_OUT, OP_LOWC, OP_GEMM };

// pointer encoding inside a plan: workspace-relative offsets (bytes) or weight-blob offsets (floats); resolved at launch time.
enum PtrSpace { PS_NULL = 0, PS_WS, PS_WEIGHT, PS_USER, PS_WINO };   // PS_WINO: off = index of a Winograd filter set of the handle
enum UserSlot { U_LABEL = 0, U_FAKE, U_PREV, U_IMG, U_MASK, U_FUSE, U_COUNT };   // U_FUSE: optional fused frame (null: no blend)
struct PRef {
  PtrSpace sp = PS_NULL;
  size_t off = 0;   // bytes for WS, floats for WEIGHT, slot id for USER
};

// A plan runs its launches in order on the caller's stream.  (Rounds 1-2 carried an option to run the condition encoder
// and the label branch on side streams: measured slower three times - two queues cost more than the overlap returns on
// this runtime - and incompatible with the lifetime-shared workspace; retired in round 3.)

// One planned launch: the fields every launch shares, a few launch selectors, the parameter struct of ITS kernel family
// with the scalar fields filled in, and one list of pointer bindings - which pointer field of that struct resolves to which
// PRef.  The bindings are the only home of a pointer: run_plan resolves them, the workspace lifetime analysis walks them
// (Builder::for_each_pref) and the byte model asks them (bound()); the pointer fields of `params` itself stay null.
using OpParams = std::variant<PackParams, IgemmParams, FinalizeParams, PoolParams, InAddParams, SplitEpiParams, ModulateParams,
                              WinoInParams, WinoOutParams, LowcParams, GemmDmaParams>;      // in the order of OpKind
static_assert(std::is_same<std::variant_alternative_t<OP_IGEMM, OpParams>, IgemmParams>::value &&
              std::is_same<std::variant_alternative_t<OP_GEMM, OpParams>, GemmDmaParams>::value, "OpParams follows OpKind");
struct Op {
  int kclass = 0;
  std::string name;
  std::string for_op;        // a finalize launch emitted on behalf of this consumer (rib_time_op times them together)
  bool label_only = false;   // depends on the label map only (pack.label, down_first, the mask network's label branch)
  dim3 grid;
  double flops = 0;
  const Variant* var = nullptr;   // k_igemm / k_gemm_dma tile
  int small_co = 0;   // > 0: a head convolution with small_co output channels: k_conv_head (matrix cores, taps as GEMM
                      //      columns) when `head`, else k_conv_small (direct, vector ALUs), instead of k_igemm
  bool head = false;
  bool fuse_blend = false;   // the mask head also writes the driver's blend into user slot U_FUSE when the caller gave one
  bool wino = false;   // this GEMM launch is the 16- / 36-way batched Winograd-domain GEMM (executes 4/9 or 1/4 of its nine-tap FLOP count)
  int wino_m = 0;      // 2 or 4 on the three launches of a Winograd convolution
  int wi_mode = 0;     // k_wino_in: WSRC_PLAIN / WSRC_SPADE / WSRC_JOIN
  int wi_mode2 = -1;   // k_wino_in with a second source (the 1x1 shortcut's input): WSRC_PLAIN / WSRC_SPADE; -1: none
  bool wi_staged = false;   // k_wino_in_staged (WinoInParams::sty x stx tiles per workgroup) instead of k_wino_in / k_wino4_in
  int lowc_ce = 0, lowc_ncol = 0, lowc_tw = 32;
  OpParams params;
  struct Binding { PRef ref; unsigned field = 0; };      // field: byte offset of the pointer inside `params`
  static constexpr int kMaxBindings = 24;            // (the largest families, k_wino_in and k_igemm, have 20 and 18 pointers)
  Binding binds[kMaxBindings];
  int nbinds = 0;

  OpKind kind() const { return (OpKind)params.index(); }
  template <class P> const P& as() const { return std::get<P>(params); }
  // a pointer field of the parameter struct P (or of a StatSrc inside it) as its byte offset; P must be this op's family
  template <class P, class T> unsigned field_of(T* P::*f) const {
    return (unsigned)(reinterpret_cast<const char*>(&(as<P>().*f)) - reinterpret_cast<const char*>(&params));
  }
  template <class P, class T> unsigned field_of(StatSrc P::*s, T* StatSrc::*f) const {
    return (unsigned)(reinterpret_cast<const char*>(&((as<P>().*s).*f)) - reinterpret_cast<const char*>(&params));
  }
  PRef ref_at(unsigned field) const {
    for (int i = 0; i < nbinds; ++i) if (binds[i].field == field) return binds[i].ref;
    return PRef();
  }
  // binding a field again replaces its reference; a null reference unbinds it
  void bind_at(unsigned field, PRef r) {
    int i = 0;
    while (i < nbinds && binds[i].field != field) ++i;
    if (r.sp == PS_NULL) { if (i < nbinds) binds[i] = binds[--nbinds]; return; }
    if (i == kMaxBindings) abort();      // (unreachable: a family has fewer pointer fields than that)
    binds[i] = Binding{r, field};
    if (i == nbinds) ++nbinds;
  }
  template <class P, class T> bool bound(T* P::*f) const { return ref_at(field_of(f)).sp != PS_NULL; }
};
// An Op under construction, typed by its kernel family: bind() takes pointer fields of P only, so a misspelt field or a
// field of another family does not compile.  push() stores the Op part.
template <class P> struct OpOf : Op {
  OpOf(int kclass_, const std::string& name_) { kclass = kclass_; name = name_; memset(&params.emplace<P>(), 0, sizeof(P)); }
  P& p() { return std::get<P>(params); }
  template <class T> void bind(T* P::*f, PRef r) { bind_at(field_of(f), r); }
  template <class T> void bind(StatSrc P::*s, T* StatSrc::*f, PRef r) { bind_at(field_of(s, f), r); }
  template <class T> PRef ref(T* P::*f) const { return ref_at(field_of(f)); }
};

// a k_stats_finalize launch not emitted yet (Norm::pend): a consumer reads the partials' place, count and affine pair from it
struct PendingStats {
  OpOf<FinalizeParams> fin;
  bool pushed = false;
  const FinalizeParams& q() const { return fin.as<FinalizeParams>(); }
  bool affine() const { return fin.bound(&FinalizeParams::gamma); }
};

struct Tap { std::string name; size_t off; int Cp, C, H, W; };

struct LazySrc;
struct Act {       // NHWC activation in the workspace
  size_t off = 0;  // bytes
  int Cp = 0, C = 0, H = 0, W = 0;
  // virt: never materialised - the channel concatenation of up to three of the caller's NCHW fp32 tensors, read in place
  // by k_conv_lowc (usrc: user slots, uc: their channel counts)
  bool virt = false; int usrc[3] = {0, 0, 0}, uc[3] = {0, 0, 0};
  // lazy: never stored - the output of an unfused SPADE (WSRC_SPADE) or of a mask-network join (WSRC_JOIN) that the
  // Winograd input transform of its only consumer computes on the fly (Builder::conv_wino)
  std::shared_ptr<LazySrc> lazy;
};
struct Norm {      // (scale, shift) arrays [B][ld]
  size_t sc = 0, sh = 0; int ld = 0;
  bool valid = false;
  // the k_stats_finalize launch that would fill the arrays, not emitted yet: a consumer that can reduce the
  // producer's partial sums itself (k_igemm prologue / SPADE epilogue, few partials) takes them from here and the
  // launch never happens; any other consumer emits it first (Builder::materialize)
  std::shared_ptr<PendingStats> pend;
};

struct LazySrc {
  int mode = 0;                 // WSRC_SPADE / WSRC_JOIN
  std::string name;             // the launch this replaces (for error messages)
  Act x; Norm nx;               // SPADE: tensor being normalised + its statistics; JOIN: t1 + n1
  bool x_ups = false, lrelu = false;
  size_t slab_off = 0; int slab_ld = 0, col0 = 0; size_t sbias_off = 0;      // SPADE: gamma/beta slab of the level, this group's bias
  bool has2 = false; Act x2; Norm n2; Act xres; Act o;                         // JOIN: ts + ns (learned shortcut) or xres; o = the stored join
};

// results of the label-only launches, as (offset, bytes) into the plan's workspace: in an autoregressive chain the
// label maps of all T frames are known up front, so rib_chain runs these launches ONCE at batch T*B (a
// labels-only plan) and copies each frame's slices into the frame plan's slots
struct LabelSlots { size_t x0 = 0, x0_b = 0, nx_sc = 0, nx_sh = 0, nx_b = 0, cat = 0, cat_b = 0, ncat_sc = 0, ncat_sh = 0, ncat_b = 0; };

struct Plan {
  bool labels_only = false;
  LabelSlots ls;
  int B, H, W;
  size_t ws_bytes = 0;
  size_t ws_virtual = 0;   // bytes before lifetime-based reuse (one range per buffer)
  std::vector<Op> ops;
  std::vector<Tap> taps;
  double flops[RIB_KC_COUNT] = {0};
};

}  // namespace
