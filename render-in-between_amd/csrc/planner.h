// planner.h — the launch planner: FusionPolicy (what is fused, which kernel family serves a layer) and Builder, which turns a
// shape into a Plan (plan.h).  A part of rib.hip's translation unit, included there once, behind the handle, the variant table
// and the weight layout; get_plan (rib.hip) is its only caller.
// Bookkeeping that the kernel families share has ONE home in Builder, and a new family goes through it, not a copy of it:
//   find_choice / tuned_choice   the tuned (variant, split-K) of a launch, its fit check and its "does not fit" error
//   bind_norm                    a light consumer's InstanceNorm source: the producer's partials, or the (scale, shift) arrays
//   alloc_partials / emit_stats  the statistics tail of a producer: partial sums, then the finalize launch, now or deferred
//   igemm_geometry / gemm_1x1    the geometry block of a k_igemm launch; a plain 1x1 GEMM as k_gemm_dma or as k_igemm
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// FusionPolicy: every decision of the launch plan that is a POLICY rather than arithmetic - which launches are fused, which
// kernel family serves a layer, where a tensor is never materialised - by name, with the switch that turns it off for an
// A/B or a test.  One instance per plan build, read from the environment at that moment (tests flip the switches between
// two Generator constructions).  Three more switches act where the weight LAYOUT is assigned, because they decide which
// filter copies exist at all (assign_weight_layout: RIB_NO_WINO, RIB_NO_LOWC, RIB_NO_SPADE16), one where the k_gemm_dma tile
// of a GEMM is picked (pick_gemm_dma: RIB_NO_DMA), one in the tile order of a grid (xcd_chunk_of: RIB_NO_XCD).
// The tuned tables (rib_set_choice) choose WITHIN what the policy allows: tile variant, split-K factor, Winograd tile.
// ------------------------------------------------------------------------------------------
struct FusionPolicy {
  // InstanceNorm statistics: a consumer that can reduce <= STATS_MAX_PARTIALS producer partials itself does so and the
  // k_stats_finalize launch never exists (RIB_NO_CONSUMER_STATS=1: one finalize launch per normalised tensor)
  bool consumer_stats = !getenv("RIB_NO_CONSUMER_STATS");
  // heads with <= 3 output channels: k_conv_head (taps as MFMA columns; RIB_NO_HEADCONV=1 -> k_conv_small, direct on the
  // vector ALUs; RIB_NO_SMALLCONV=1 -> k_igemm with the columns padded to 16)
  bool head_conv = !getenv("RIB_NO_HEADCONV");
  bool small_conv = !getenv("RIB_NO_SMALLCONV");
  // 3x3 stride-1 layers on maps of at most this many pixels run in the Winograd domain (k_wino_in / batched GEMM / k_wino_out)
  long wino_max_px = getenv("RIB_WINO_MAX_PX") ? atol(getenv("RIB_WINO_MAX_PX")) : 16384;
  int wino_force = getenv("RIB_WINO_M") ? atoi(getenv("RIB_WINO_M")) : 0;      // 2 / 4: that Winograd tile wherever one is eligible
  // grid-level split-K (+ a k_splitk_epilogue launch) for layers whose tile grid cannot fill the chip
  bool split_k = !getenv("RIB_NO_SPLITK");
  // layers with <= 16 output channels on the 16-column MFMA path (v_mfma_f32_16x16x4_f32; fp32 storage only)
  bool n16 = !getenv("RIB_NO_N16");
  // k_conv_lowc tile width: 0 = per layer (16 for the store-bound 64-column layer without statistics, else 32)
  int lowc_tw = getenv("RIB_LOWC_TW") ? (atoi(getenv("RIB_LOWC_TW")) == 16 ? 16 : 32) : 0;
  // condition levels of at most this many pixels compute gamma/beta of ALL their SPADEs in one GEMM into a slab (0: off)
  long cond_gemm_max_px = getenv("RIB_COND_GEMM_MAX_PX") ? atol(getenv("RIB_COND_GEMM_MAX_PX")) : 4096;
  // SPADE on maps of <= 4096 pixels (x batch): unfused (slab GEMM + k_spade_modulate) instead of k_igemm<SPADE>
  bool unfused_spade = !getenv("RIB_NO_UNFUSED_SPADE");
  // an unfused SPADE's output / a mask-network join whose only consumer is a Winograd input transform is never stored
  bool lazy_sources = !getenv("RIB_NO_LAZY");
  // the learned 1x1 shortcut of a res block as extra K chunks of conv_block_1 (one launch less, no shortcut tensor)
  bool fuse_shortcut = !getenv("RIB_NO_FUSE_SHORTCUT");
  // conv_block_1 of a learned-shortcut block in the Winograd domain, the shortcut as extra K columns at the centre-tap positions
  // (Builder::shortcut_wino_m).  On only where the tuned table has an entry for the layer's .wino / .wino4 launch - shapes nobody
  // measured keep the direct launch; RIB_NO_WINO_SHORTCUT=1: nowhere; RIB_WINO_SHORTCUT_M=2 / 4: wherever eligible, that tile
  bool wino_shortcut = !getenv("RIB_NO_WINO_SHORTCUT");
  int wino_shortcut_m = getenv("RIB_WINO_SHORTCUT_M") ? atoi(getenv("RIB_WINO_SHORTCUT_M")) : 0;
  // buffers with disjoint lifetimes share workspace bytes (assign_physical)
  bool ws_reuse = !getenv("RIB_NO_WS_REUSE");
  // level i of the mask network's label encoder and of its image encoder in ONE paired launch (batch-1 frame plans).
  // Asked on every forward, ahead of the plan cache (plan_pairs): a function of its own, so that asking reads this switch alone
  static bool pair_mask_encoders() { return !getenv("RIB_NO_PAIR"); }
};

struct Builder {
  rib_handle* h;
  Plan* P;
  int B;
  const FusionPolicy pol;
  size_t ws = 0;
  std::string error;
  bool mark_label = false;
  bool pair_mask = false;    // the two encoders of the mask network level by level in paired launches (mask_branches_paired)
  bool defer_stats = true;   // false: every k_stats_finalize launch is emitted where its producer is (labels-only plans)
  // a consumer needs the (scale, shift) ARRAYS of n: emit the finalize launch now if it is still pending
  void materialize(const Norm& n, const std::string& consumer = std::string()) {
    if (n.pend && !n.pend->pushed) { n.pend->pushed = true; n.pend->fin.for_op = consumer; push(n.pend->fin); }
  }
  // the producer's partial sums are still there for a consumer-side finalize
  static bool has_partials(const Norm& n) { return n.pend && !n.pend->pushed; }
  // ... plain ones (no affine pair), of at least Cp columns: what the SPADE kernels can reduce
  static bool has_plain_partials(const Norm& n, int Cp) { return has_partials(n) && !n.pend->affine() && Cp <= n.pend->q().Cs; }
  // emit the finalize launch f of a producer, or leave it to the consumers of *out (at most STATS_MAX_PARTIALS partials)
  void finalize_or_defer(const OpOf<FinalizeParams>& f, Norm* out, bool now) {
    if (now || !pol.consumer_stats || !defer_stats || mark_label || f.as<FinalizeParams>().tiles > STATS_MAX_PARTIALS) push(f);
    else out->pend = std::make_shared<PendingStats>(PendingStats{f});
  }
  // A light consumer (k_wino_in, k_spade_modulate, k_in_add: channel slices of 64) reduces the producer's partials itself:
  // fills the scalars of the op's StatSrc `src` and binds its pointers from the pending finalize of n, which then never
  // launches unless another consumer needs the arrays.  false: the partials are gone or the launch was forced -> the caller
  // materializes (bind_norm).
  template <class P> bool take_partials(const Norm& n, OpOf<P>& op, StatSrc P::*src) {
    if (!has_partials(n)) return false;
    const OpOf<FinalizeParams>& f = n.pend->fin;
    StatSrc& st = op.p().*src;
    st.tiles = n.pend->q().tiles; st.Cs = n.pend->q().Cs; st.inv_count = n.pend->q().inv_count;
    op.bind(src, &StatSrc::part, f.ref(&FinalizeParams::part));
    if (n.pend->affine()) { op.bind(src, &StatSrc::gamma, f.ref(&FinalizeParams::gamma)); op.bind(src, &StatSrc::beta, f.ref(&FinalizeParams::beta)); }
    return true;
  }
  // The InstanceNorm source n of a light consumer `op`: the producer's partials through the StatSrc `st` where `partials` allows
  // and they are still there (true), else the finalize launch is materialized on behalf of `consumer` and the (scale, shift) arrays
  // are bound, from channel choff on (false).  (Apart: the igemm prologue never takes partials, the SPADE epilogue has no StatSrc.)
  template <class P, class T> bool bind_norm(OpOf<P>& op, const Norm& n, const std::string& consumer, StatSrc P::*st, T* P::*scale, T* P::*shift,
                                             bool partials = true, size_t choff = 0) {
    if (partials && take_partials(n, op, st)) return true;
    materialize(n, consumer);
    op.bind(scale, WS(n.sc + choff * sizeof(float))); op.bind(shift, WS(n.sh + choff * sizeof(float)));
    return false;
  }
  // the k_stats_finalize launch of a producer that left `tiles` partial sums per image (Cs columns, C of them stored) at part_off
  OpOf<FinalizeParams> finalize_op(const std::string& producer, size_t part_off, int tiles, int Cs, int C, const Norm& out, size_t choff,
                                   int H, int W, const ConvDef* affine, int images) {
    OpOf<FinalizeParams> f(RIB_KC_STATS, producer + ".stats");
    FinalizeParams& q = f.p();
    q.tiles = tiles; q.Cs = Cs; q.C = C; q.ld = out.ld; q.off = (int)choff;
    q.inv_count = 1.0f / ((float)H * (float)W); q.eps = 1e-5f;
    f.bind(&FinalizeParams::part, WS(part_off));
    if (affine) { f.bind(&FinalizeParams::gamma, WT(affine->g_off)); f.bind(&FinalizeParams::beta, WT(affine->be_off)); }
    f.bind(&FinalizeParams::scale, WS(out.sc)); f.bind(&FinalizeParams::shift, WS(out.sh));
    f.grid = dim3((Cs + 15) / 16, images, 1);
    return f;
  }
  // the statistics partials a producer leaves: `tiles` (sum, sum of squares) pairs of coutp doubles per image
  size_t alloc_partials(int images, int tiles, int coutp) { return alloc((size_t)images * tiles * 2 * coutp * sizeof(double)); }
  // gamma/beta slab of a condition level (cond_level_gemm): [B][H*W][ld] fp32, group columns at SpadeGroup::col0
  struct LevelSlab { size_t off = 0; int ld = 0; };
  std::map<int, LevelSlab> level_slab;
  int tuneB = 0;      // batch whose tuned choices / cost-model decisions this plan follows (0: its own).  The labels-only
                      // plan of a chain follows the frame plan's, so that its results are bit-identical to per-frame launches
  int TB_() const { return tuneB > 0 ? tuneB : B; }
  void push(Op op) {
    op.label_only = mark_label;
    P->ops.push_back(op);
  }

  // Workspace layout.  During the build every buffer gets its own range of a virtual address space (bump
  // allocation, as the plan used to run: 1.1 GB at 512x512); assign_physical() then gives buffers whose lifetimes
  // (first .. last launch that touches them) do not overlap the same bytes, so that the working set of a frame stays
  // inside the 256 MB memory-side cache instead of streaming 1.1 GB of distinct addresses through it.
  struct AllocRec { size_t voff, bytes, phys; int first, last; };
  std::vector<AllocRec> allocs;
  size_t alloc(size_t bytes) {
    size_t o = ws; ws += align256(bytes);
    allocs.push_back(AllocRec{o, align256(bytes), o, INT_MAX, -1});
    return o;
  }
  Act act(int C, int H, int W) { return act_n(B, C, H, W); }
  Norm norm(int Cp, int images = 0) {
    Norm n; n.ld = Cp; n.valid = true;
    n.sc = alloc((size_t)(images ? images : B) * Cp * sizeof(float));
    n.sh = alloc((size_t)(images ? images : B) * Cp * sizeof(float));
    return n;
  }
  Act act_n(int images, int C, int H, int W) {     // an activation of `images` images instead of B
    Act a; a.C = C; a.Cp = h->padc(C); a.H = H; a.W = W;
    a.off = alloc((size_t)images * H * W * a.Cp * h->esz());
    return a;
  }
  // an activation that is never materialised: up to three of the caller's NCHW tensors, concatenated along channels
  Act virt(int C, int H, int W, int s0, int c0, int s1 = 0, int c1 = 0, int s2 = 0, int c2 = 0) {
    Act a; a.virt = true; a.C = C; a.Cp = 0; a.H = H; a.W = W;
    a.usrc[0] = s0; a.uc[0] = c0; a.usrc[1] = s1; a.uc[1] = c1; a.usrc[2] = s2; a.uc[2] = c2;
    return a;
  }
  // the pack launch: one or two of the caller's NCHW tensors (c0 + c1 channels) into the NHWC activation dst, padding zeroed
  void pack(const std::string& nm, const Act& dst, int s0, int c0, int s1 = 0, int c1 = 0) {
    OpOf<PackParams> op(RIB_KC_PACK, nm);
    op.p().c0 = c0; op.p().c1 = c1; op.p().dC = dst.Cp; op.p().HW = dst.H * dst.W;
    op.bind(&PackParams::s0, US(s0)); if (c1) op.bind(&PackParams::s1, US(s1));
    op.bind(&PackParams::dst, WS(dst.off));
    op.grid = dim3((dst.H * dst.W + 63) / 64, B, 1);
    push(op);
  }
  // every consumer of a packed input tensor has a k_conv_lowc instantiation
  bool lowc_serves(std::initializer_list<const char*> names) {
    for (const char* nm : names) {
      auto it = h->conv_index.find(nm);
      if (it == h->conv_index.end() || !h->convs[it->second].wl_off) return false;
    }
    return true;
  }
  // conv_img can skip its NHWC copy only on the head kernel (conv(): `small` + `head`)
  bool head_without_nhwc(const ConvDef& c) {
    return c.cout <= 3 && c.ks == 3 && c.stride == 1 && (c.cinp == 16 || c.cinp == 32) && pol.small_conv && pol.head_conv;
  }
  static PRef WS(size_t off) { PRef r; r.sp = PS_WS; r.off = off; return r; }
  static PRef WT(size_t off) { PRef r; r.sp = PS_WEIGHT; r.off = off; return r; }
  static PRef US(int slot) { PRef r; r.sp = PS_USER; r.off = (size_t)slot; return r; }
  static PRef WINO(int set) { PRef r; r.sp = PS_WINO; r.off = (size_t)set; return r; }
  void tap(const std::string& name, const Act& a) { P->taps.push_back(Tap{name, a.off, a.Cp, a.C, a.H, a.W}); }

  // ---- generic convolution launch --------------------------------------------------------
  struct ConvArgs {
    const ConvDef* cd = nullptr;
    Act in;                 // input activation (stored size; half-res when ups)
    bool ups = false;
    const Norm* pro = nullptr; size_t pro_choff = 0;   // prologue affine (+channel offset into the arrays)
    bool pro_lrelu = false;
    Act out; int yoff = 0;  // destination buffer and channel offset
    int cout_store = -1;    // columns stored (default: out slice padded width)
    int act = ACT_NONE;
    const Act* res = nullptr; bool res_ups = false;
    const ConvDef* aux = nullptr; Act aux_in;   // fused 1x1 shortcut operand (accumulated into the same output)
    PRef y_nchw;            // optional NCHW copy
    PRef y_user;            // when set, y is this user tensor (yC = cout exactly)
    bool y_none = false;    // no NHWC destination at all (a head that only writes its NCHW copy)
    bool want_stats = false;
    Norm* stats_out = nullptr; size_t stats_choff = 0;  // finalize target (+channel offset)
    bool affine = false;    // finalize with the conv's IN gamma/beta
    bool stats_now = false; // emit the finalize launch at the producer (the arrays are shared / copied between plans)
    // Two convolutions of identical shape in one launch (IgemmParams::pair): `pair` is the second one; `in` / `out` hold
    // 2B images (image 2b + j belongs to convolution j).  pair_merge: the outputs of a pair land in ONE image of `out`
    // (B images) at channel offsets yoff and yoff + pair_yoff, and their statistics in one row of stats_out.
    const ConvDef* pair = nullptr; bool pair_merge = false; int pair_yoff = 0;
    bool no_split = false;              // never grid-level split-K (the paired launch cannot, and its unpaired twins must match it)
    std::vector<std::string> choice_names;   // tuned-choice keys tried before the op's own name
  };

  // ---- what the kernel families share: algorithmic FLOP count of convolution c on n output maps of H x W, and of the gamma/beta GEMM of a SPADE group (batch B)
  static double conv_flops(const ConvDef& c, int H, int W, int n) { return 2.0 * c.cin * c.ks * c.ks * c.cout * (double)H * W * n; }
  double spade_flops(const SpadeGroup& sg, int H, int W) const { return 2.0 * sg.cond * 2.0 * sg.nsets * sg.C * (double)H * W * B; }
  // output columns a convolution stores into its NHWC destination
  int stored_cout(const ConvArgs& a, const ConvDef& c) const { return a.cout_store >= 0 ? a.cout_store : h->padc(c.cout); }
  bool out_fits(const ConvArgs& a, const std::string& opname, int Hout, int Wout) {
    if (a.out.H == Hout && a.out.W == Wout) return true;
    error = fmt("%s: output size mismatch", opname.c_str());
    return false;
  }
  // Statistics tail of a convolution that left `tiles` partials per image at part_off: its finalize launch, emitted here or
  // deferred to the consumers of a.stats_out.  (A channel offset means two producers share the arrays - the concatenated
  // encoders of the mask network - and consumers would need two partial sources: those keep their launch; so does a paired launch)
  void emit_stats(const std::string& opname, const ConvArgs& a, size_t part_off, int tiles, int Hout, int Wout, int images) {
    const ConvDef& c = *a.cd;
    OpOf<FinalizeParams> f = finalize_op(opname, part_off, tiles, c.coutp, h->padc(c.cout), *a.stats_out, a.stats_choff, Hout, Wout, a.affine ? &c : nullptr, images);
    if (a.pair) { f.p().g_stride = a.affine ? (int)(a.pair->g_off - c.g_off) : 0; f.p().pair_merge = a.pair_merge ? 1 : 0; f.p().pair_off = a.pair_yoff; }
    finalize_or_defer(f, a.stats_out, a.stats_choff != 0 || a.stats_now || a.pair != nullptr);
  }
  // tuned choices (rib_set_choice) are keyed by the followed batch, the frame size and a launch's name
  std::string choice_key(const std::string& name) const { return fmt("%d,%d,%d|%s", TB_(), P->H, P->W, name.c_str()); }
  // the tuned (variant index, split-K) of the first of `names` that has one
  const std::pair<int, int>* find_choice(const std::vector<std::string>& names) const {
    for (const std::string& nm : names) {
      auto it = h->choices.find(choice_key(nm));
      if (it != h->choices.end()) return &it->second;
    }
    return nullptr;
  }
  // ... into *ch (untouched without one) if fits(variant, ksplit).  false: it does not fit - `error` says so for `who`, the build fails
  template <class Fit> bool tuned_choice(const std::vector<std::string>& names, const std::string& who, const char* what, Choice* ch, Fit fits) {
    const std::pair<int, int>* t = find_choice(names);
    if (t && !fits(kVariants[t->first], t->second)) { error = fmt("%s: tuned choice (variant %d, ksplit %d) does not fit this %s", who.c_str(), t->first, t->second, what); return false; }
    if (t) { ch->v = &kVariants[t->first]; ch->ksplit = t->second; }
    return true;
  }
  // Geometry block of a k_igemm launch on tile variant v: input map as stored (xC channels per pixel, Cin of them read), output map,
  // padded columns, split-K factor, tile grid (phase-decomposed upsample convolution: tiles of SOURCE pixels, a 2TH x 2TW patch each)
  static void igemm_geometry(IgemmParams& p, const Variant* v, int Hin, int Win, int xC, int Cin, int CoutPad, int Hout, int Wout, int ksplit = 1, bool ups = false) {
    p.Hin = Hin; p.Win = Win; p.xC = xC; p.Cin = Cin; p.CoutPad = CoutPad; p.Hout = Hout; p.Wout = Wout; p.ksplit = ksplit;
    p.tilesX = ((ups ? Win : Wout) + v->TW() - 1) / v->TW(); p.tilesY = ((ups ? Hin : Hout) + v->TH() - 1) / v->TH();
    p.xcd_chunk = xcd_chunk_of(p.tilesX * p.tilesY);
  }
  // One plain GEMM launch on tile v - Z problems of (H*W) x N x K, rows of A `lda` apart - in the form v serves: k_gemm_dma, or k_igemm
  // as a 1x1 convolution of Z images of an H x W map.  nsets > 0: problem z reads filter set z % nsets (Winograd positions), the result
  // is a plain tensor; 0: one filter matrix, the result a split-K slab (gamma/beta).  K2 / kmask: the fused shortcut's K extent
  // (k_gemm_dma only).  Returned, not pushed: the caller adds what is its own.
  struct Gemm1x1 { PRef a, w, c, bias; int Z = 1, H = 0, W = 0, K = 0, N = 0, lda = 0, nsets = 0, ksplit = 1, K2 = 0; unsigned long long kmask = 0; };
  Op gemm_1x1(int kclass, const std::string& name, const Variant* v, const Gemm1x1& m, double flops) {
    const int M = m.H * m.W;
    if (v->dma()) {
      OpOf<GemmDmaParams> op(kclass, name); op.var = v; op.flops = flops;
      GemmDmaParams& g = op.p();
      g.M = M; g.N = m.N; g.K = m.K; g.lda = m.lda; g.ldc = m.N;
      g.sA = (size_t)M * m.lda; g.sB = m.nsets ? (size_t)m.N * m.lda : 0; g.sC = (size_t)M * m.N; g.modB = m.nsets;
      g.K2 = m.K2; g.kmask = m.kmask;
      op.bind(&GemmDmaParams::A, m.a); op.bind(&GemmDmaParams::B, m.w); op.bind(&GemmDmaParams::C, m.c);
      op.grid = dim3((M + v->BM() - 1) / v->BM(), (m.N + v->BN() - 1) / v->BN(), m.Z);
      return op;
    }
    OpOf<IgemmParams> op(kclass, name); op.var = v; op.flops = flops;
    IgemmParams& p = op.p();
    igemm_geometry(p, v, m.H, m.W, m.lda, m.K, m.N, m.H, m.W, m.ksplit);
    op.bind(&IgemmParams::x, m.a); op.bind(&IgemmParams::w, m.w); op.bind(&IgemmParams::bias, m.bias);
    if (m.nsets) {
      p.act = ACT_NONE; p.yC = m.N; p.yoff = 0; p.Cout = m.N; p.w_mod = m.nsets; p.w_stride = (unsigned)((size_t)m.N * m.K);
      op.bind(&IgemmParams::y, m.c);
    } else op.bind(&IgemmParams::slab, m.c);
    op.grid = dim3(p.tilesX * p.tilesY, (m.N + v->BN() - 1) / v->BN(), m.Z * m.ksplit);
    return op;
  }

  // Winograd F(2x2, 3x3) / F(4x4, 3x3) on the small maps (k_wino_in / batched 1x1 k_igemm / k_wino_out; kernels.hip.h):
  // maps up to 128x128 (1024x1024 frames: +3.5 % at batch 1 and 4); beyond that V and M (4x the activation each)
  // leave the caches and the direct kernel, which fills the chip there, was not beaten
  // (opname: of a convolution with a fused shortcut - the tuned table decides for those, shortcut_wino_m)
  bool runs_wino(const ConvArgs& a, int Hout, int Wout, const std::string& opname = std::string()) const {
    const ConvDef& c = *a.cd;
    return h->prec() == PREC_F32 && (a.aux ? c.wino_s_ok : c.wino_ok) && !a.ups && !a.res_ups && !a.pair && !a.in.virt && a.y_nchw.sp == PS_NULL &&
           a.y_user.sp == PS_NULL && (long)Hout * Wout <= pol.wino_max_px && Hout >= 2 && Wout >= 2 &&
           (!a.aux || (!a.res && shortcut_wino_m(c, *a.aux, opname, Hout, Wout) != 0));
  }
  // F(4x4, 3x3) where its per-position GEMM still has >= 256 rows (conv_wino), else F(2x2, 3x3)
  int default_wino_m(int Hout, int Wout) const { return (long)TB_() * ((Hout + 3) / 4) * ((Wout + 3) / 4) >= 256 ? 4 : 2; }
  // Winograd tile (2 / 4) of a 3x3 convolution with its learned 1x1 shortcut fused in, 0: it stays a direct launch.  The cost
  // model keeps the direct launch; a tuned entry for "<op>.wino" or "<op>.wino4" of this shape (its variant: the GEMM tile)
  // switches the layer over.  The batched GEMM with a K extent per position exists in k_gemm_dma only.
  int shortcut_wino_m(const ConvDef& c, const ConvDef& s, const std::string& opname, int Hout, int Wout) const {
    if (!pol.wino_shortcut || !pol.fuse_shortcut || opname.empty() || !c.fb_off || s.ks != 1 || s.coutp != c.coutp || s.cinp % 32 != 0 || c.cinp % 32 != 0) return 0;
    if (!pick_gemm_dma(h->prec(), 16, 64, c.coutp, c.cinp)) return 0;
    if (pol.wino_shortcut_m == 2 || pol.wino_shortcut_m == 4) return pol.wino_shortcut_m;
    const int d = default_wino_m(Hout, Wout);
    for (int m : {d, 6 - d})
      if (find_choice({opname + (m == 2 ? ".wino" : ".wino4")})) return m;
    return 0;
  }
  // would conv `cd` on an HxW map (stride 1, plain arguments) run in the Winograd domain?  (callers that want to hand it a lazy input)
  bool would_wino(const ConvDef& cd, int H, int W) const { ConvArgs t; t.cd = &cd; return runs_wino(t, H, W); }

  bool conv(const ConvArgs& a, const std::string& opname) {
    const ConvDef& c = *a.cd;
    const int Hout = a.ups ? a.in.H * 2 : (c.stride == 2 ? a.in.H / 2 : a.in.H);
    const int Wout = a.ups ? a.in.W * 2 : (c.stride == 2 ? a.in.W / 2 : a.in.W);
    if (a.in.virt) return conv_lowc(a, opname);
    const int nB = a.pair ? 2 * B : B;       // images in `in`
    if (a.pair) {
      const ConvDef& d = *a.pair;
      if (d.cinp != c.cinp || d.coutp != c.coutp || d.cout != c.cout || d.ks != c.ks || d.stride != c.stride || d.ups_in || c.ups_in || a.ups || a.res || a.aux ||
          a.y_nchw.sp != PS_NULL || a.y_user.sp != PS_NULL || a.y_none || !a.want_stats || c.in_affine != d.in_affine || d.w_off <= c.w_off || d.b_off <= c.b_off ||
          (c.in_affine && (d.g_off <= c.g_off || d.g_off - c.g_off != d.be_off - c.be_off)) || (h->mc16() && d.w16_off <= c.w16_off)) {
        error = opname + ": the two convolutions of a paired launch must have the same shape"; return false;
      }
    }
    if (a.in.Cp != c.cinp) { error = fmt("%s: input channels %d != expected %d", opname.c_str(), a.in.Cp, c.cinp); return false; }
    if (runs_wino(a, Hout, Wout, opname)) return conv_wino(a, opname, Hout, Wout);
    if (a.in.lazy) { error = opname + ": a lazy input (" + a.in.lazy->name + ") needs the Winograd path"; return false; }
    if (a.aux && a.aux_in.lazy) { error = opname + ": a lazy shortcut input (" + a.aux_in.lazy->name + ") needs the Winograd path"; return false; }
    // split-K needs the slab-summing epilogue: float4 channel groups that tile a 256-thread block,
    // and no NCHW side copy
    const bool can_split = (256 % (c.coutp / 4) == 0) && a.y_nchw.sp == PS_NULL && !a.pair && !a.no_split && pol.split_k;
    // the 16-column path serves layers with <= 16 output channels and no residual read
    const bool can_n16 = c.cout <= 16 && !a.res && !h->mc16() && pol.n16;
    Choice ch = choose_variant(h->prec(), c.stride, c.ks, a.ups, false, c.coutp, TB_(), Hout, Wout, c.cinp, can_split, a.aux ? a.aux->cinp : 0, can_n16);
    std::vector<std::string> names = a.choice_names;
    names.push_back(opname);
    if (!tuned_choice(names, opname, "layer", &ch, [&](const Variant& tv, int ts) {
          return !tv.dma() && !(tv.DMAK && (a.aux || ts != 1)) && !(tv.DMAK && !tv.fn_pro && !tv.fn && (a.pro || a.pro_lrelu)) && tv.BF16 == h->prec() && tv.STRIDE == c.stride && tv.KS == c.ks && tv.UPS == a.ups && !tv.SPADE && c.cinp % tv.BK == 0 &&
                 (!a.aux || a.aux->cinp % tv.BK == 0) && (tv.NF != 0 || (can_n16 && ts == 1)) &&
                 ts >= 1 && ts <= c.cinp / tv.BK && (ts == 1 || can_split);
        })) return false;
    const Variant* v = ch.v;
    if (!v) { error = fmt("%s: no kernel variant for Cin=%d stride=%d ks=%d ups=%d", opname.c_str(), c.cinp, c.stride, c.ks, (int)a.ups); return false; }
    const int S = ch.ksplit;
    OpOf<IgemmParams> op(RIB_KC_IGEMM, opname); op.var = v;
    IgemmParams& p = op.p();
    igemm_geometry(p, v, a.in.H, a.in.W, a.in.Cp, c.cinp, c.coutp, Hout, Wout, S, a.ups);
    p.pro_ld = a.pro ? a.pro->ld : 0; p.pro_lrelu = a.pro_lrelu ? 1 : 0;
    if (a.ups && (!c.ups_in || c.ks != 3 || c.stride != 1)) { error = opname + ": no phase filters for this upsample convolution"; return false; }
    p.act = a.act;
    op.bind(&IgemmParams::x, WS(a.in.off));
    // heads with 1..4 output channels (conv_img, conv_mask.0): direct convolution on the vector ALUs; the
    // matrix-core kernels would pad N to 16 columns.  y_nchw's channel count is Cout of the conv itself.
    const bool small = c.cout <= 4 && c.ks == 3 && c.stride == 1 && !a.ups && !a.res && !a.aux && !a.want_stats &&
                       c.cinp <= 32 && 256 % (c.cinp / 4) == 0 &&   // halo tile + filter within the default 64 KB of dynamic LDS
                       pol.small_conv;
    if (a.pro) {
      // (a consumer-side finalize in the PROLOGUE was tried and removed: its (scale, shift) table cost every prologue
      // variant 4 KB of LDS - an occupancy step for several of them - to save four launches; the SPADE epilogue keeps its own)
      materialize(*a.pro, opname);
      op.bind(&IgemmParams::pro_scale, WS(a.pro->sc + a.pro_choff * sizeof(float)));
      op.bind(&IgemmParams::pro_shift, WS(a.pro->sh + a.pro_choff * sizeof(float)));
    }
    // matrix-core kernels of a bf16 handle read the bf16 filter copies; the direct head convolutions keep fp32 filters
    const bool w16 = h->mc16() && !small;
    op.bind(&IgemmParams::w, WT(a.ups ? (w16 ? c.wp16_off : c.wp_off) : (w16 ? c.w16_off : c.w_off))); op.bind(&IgemmParams::bias, WT(c.b_off));
    double aux_flops = 0.0;
    if (a.aux) {
      if (c.ks != 3 || c.stride != 1 || a.ups || !c.fb_off || a.aux->ks != 1 || a.aux->coutp != c.coutp || a.aux_in.Cp != a.aux->cinp ||
          a.aux_in.H != Hout || a.aux_in.W != Wout) { error = opname + ": fused shortcut operand does not fit"; return false; }
      op.bind(&IgemmParams::x2, WS(a.aux_in.off)); op.bind(&IgemmParams::w2, WT(h->mc16() ? a.aux->w16_off : a.aux->w_off)); op.bind(&IgemmParams::bias, WT(c.fb_off));
      p.x2C = a.aux_in.Cp; p.Cin2 = a.aux->cinp;
      aux_flops = conv_flops(*a.aux, Hout, Wout, B);
    }
    if (a.y_user.sp != PS_NULL) {
      op.bind(&IgemmParams::y, a.y_user); p.yC = c.cout; p.yoff = 0; p.Cout = c.cout; p.y_f32 = 1;   // a caller's fp32 tensor
    } else if (a.y_none) {
      p.yC = 0; p.yoff = 0; p.Cout = a.cout_store >= 0 ? a.cout_store : c.cout;
    } else {
      op.bind(&IgemmParams::y, WS(a.out.off)); p.yC = a.out.Cp; p.yoff = a.yoff;
      p.Cout = stored_cout(a, c);
      if (!out_fits(a, opname, Hout, Wout)) return false;
    }
    if (a.pair) {
      const bool w16p = h->mc16();
      p.w_mod = 2;
      p.w_stride = (unsigned)(w16p ? 2 * (a.pair->w16_off - c.w16_off) : a.pair->w_off - c.w_off);      // elements of the filter's storage type
      p.b_stride = (unsigned)(a.pair->b_off - c.b_off);
      p.pair = a.pair_merge ? 1 : 0; p.pair_yoff = a.pair_yoff;
    }
    if (a.res) { op.bind(&IgemmParams::res, WS(a.res->off)); p.resC = a.res->Cp; p.res_ups = a.res_ups ? 1 : 0; }
    op.bind(&IgemmParams::y_nchw, a.y_nchw);
    if (a.y_none && !(small && c.cout <= 3 && (c.cinp == 16 || c.cinp == 32) && pol.head_conv && a.y_nchw.sp != PS_NULL)) {
      error = opname + ": only the head kernel can run without an NHWC destination"; return false;
    }
    if (small) {
      op.small_co = c.cout;
      op.head = c.cout <= 3 && (c.cinp == 16 || c.cinp == 32) && pol.head_conv;
      // the mask head has every pixel's mask in a register: the driver's blend (evaluator.py:256-258) rides along
      op.fuse_blend = op.head && c.cout == 1 && a.y_user.sp == PS_USER && a.y_user.off == (size_t)U_MASK;
      p.bl_C = h->g.c.image_nc;
      p.ksplit = 1;
      p.tilesX = (Wout + 15) / 16; p.tilesY = (Hout + 15) / 16; p.xcd_chunk = xcd_chunk_of(p.tilesX * p.tilesY);
      op.grid = dim3(p.tilesX * p.tilesY, 1, B);
      op.flops = conv_flops(c, Hout, Wout, B);
      P->flops[RIB_KC_IGEMM] += op.flops;
      push(op);
      return true;
    }
    int tiles = p.tilesX * p.tilesY;
    size_t part_off = 0;
    op.grid = dim3(tiles, v->NF == 0 ? 1 : (c.coutp + v->BN() - 1) / v->BN(), nB * S);
    op.flops = conv_flops(c, Hout, Wout, nB) + aux_flops;
    P->flops[RIB_KC_IGEMM] += op.flops;
    if (a.pair && (S != 1 || v->NF == 0)) { error = opname + ": a paired launch cannot split K or use the 16-column path"; return false; }
    if (S == 1) {
      if (a.want_stats) { part_off = alloc_partials(nB, tiles, c.coutp); op.bind(&IgemmParams::stat_part, WS(part_off)); }
      push(op);
    } else {
      // split-K: the conv writes raw partial slabs; a second kernel sums them and runs the epilogue
      const size_t slab_off = alloc((size_t)S * B * Hout * Wout * c.coutp * sizeof(float));
      op.bind(&IgemmParams::slab, WS(slab_off));
      OpOf<SplitEpiParams> e(RIB_KC_CONVAUX, opname + ".splitk_sum");
      SplitEpiParams& q = e.p();
      q.ksplit = S; q.B = B; q.CoutPad = c.coutp; q.yC = p.yC; q.yoff = p.yoff; q.Cout = p.Cout;
      q.act = p.act; q.resC = p.resC; q.res_ups = p.res_ups; q.Hout = Hout; q.Wout = Wout;
      const int slots = 256 / (c.coutp / 4), ppb = slots * 4;
      const int blocks = (Hout * Wout + ppb - 1) / ppb;
      q.blocks = blocks;
      // the epilogue launch takes over the convolution's bias, destination and residual
      e.bind(&SplitEpiParams::slab, WS(slab_off)); e.bind(&SplitEpiParams::bias, op.ref(&IgemmParams::bias));
      e.bind(&SplitEpiParams::y, op.ref(&IgemmParams::y)); e.bind(&SplitEpiParams::res, op.ref(&IgemmParams::res));
      if (a.want_stats) { part_off = alloc_partials(B, blocks, c.coutp); e.bind(&SplitEpiParams::stat_part, WS(part_off)); }
      e.grid = dim3(blocks, B, 1);
      tiles = blocks;   // the statistics partials now come from the epilogue kernel's blocks
      op.bind(&IgemmParams::y, PRef()); op.bind(&IgemmParams::res, PRef());
      push(op);
      push(e);
    }
    if (a.want_stats) emit_stats(opname, a, part_off, tiles, Hout, Wout, nB);
    return true;
  }

  // first-layer 3x3 convolution over the caller's NCHW tensors (k_conv_lowc): no packed copy, reduction over the real channels
  bool conv_lowc(const ConvArgs& a, const std::string& opname) {
    const ConvDef& c = *a.cd;
    const int H = a.in.H, W = a.in.W;
    if (!c.wl_off || c.ks != 3 || c.stride != 1 || a.ups || a.pro || a.res || a.aux || a.y_nchw.sp != PS_NULL || a.y_user.sp != PS_NULL ||
        a.in.uc[0] + a.in.uc[1] + a.in.uc[2] != c.cin) { error = opname + ": not a layer k_conv_lowc can run"; return false; }
    if (!out_fits(a, opname, H, W)) return false;
    OpOf<LowcParams> op(RIB_KC_IGEMM, opname); op.lowc_ce = c.lowc_ce; op.lowc_ncol = c.lowc_ncol;
    LowcParams& p = op.p();
    p.c0 = a.in.uc[0]; p.c1 = a.in.uc[1]; p.c2 = a.in.uc[2];
    p.H = H; p.W = W; p.yC = a.out.Cp; p.yoff = a.yoff; p.Cout = stored_cout(a, c);
    p.act = a.act; p.CoutPad = c.coutp;
    // 8x16 tiles (2048 workgroups at 512x512: two rounds, whose gather / MFMA / store phases overlap) win where the layer is
    // store-bound and has no statistics (conv_first 44.6 -> 38.4 us); with statistics the finalize of twice the partials
    // eats the gain (down_lbl.0 -3 +3 us) and the 16-column layer loses (29.5 -> 32.7)
    const int tw = pol.lowc_tw ? pol.lowc_tw : ((c.lowc_ncol == 64 && !a.want_stats) ? 16 : 32);
    op.lowc_tw = tw;
    p.tilesX = (W + tw - 1) / tw; p.tilesY = (H + 7) / 8;
    if (p.Cout > c.lowc_ncol || c.cout > c.lowc_ncol) { error = opname + ": more output columns than the k_conv_lowc instantiation has"; return false; }
    op.bind(&LowcParams::s0, US(a.in.usrc[0])); if (p.c1) op.bind(&LowcParams::s1, US(a.in.usrc[1])); if (p.c2) op.bind(&LowcParams::s2, US(a.in.usrc[2]));
    op.bind(&LowcParams::w, WT(c.wl_off)); op.bind(&LowcParams::bias, WT(c.b_off)); op.bind(&LowcParams::y, WS(a.out.off));
    const int tiles = p.tilesX * p.tilesY;
    size_t part_off = 0;
    if (a.want_stats) { part_off = alloc_partials(B, tiles, c.coutp); op.bind(&LowcParams::stat_part, WS(part_off)); }
    op.grid = dim3(tiles, B, 1);
    op.flops = conv_flops(c, H, W, B);
    P->flops[RIB_KC_IGEMM] += op.flops;
    push(op);
    if (a.want_stats) emit_stats(opname, a, part_off, tiles, H, W, B);
    return true;
  }

  bool conv_wino(const ConvArgs& a, const std::string& opname, int Hout, int Wout) {
    const ConvDef& c = *a.cd;
    // F(4x4, 3x3) (36 positions, 1/4 of the multiplications) where its per-position GEMM still has >= 256 rows (maps of
    // 64x64 and more at batch 1); below that the 36 GEMMs are filter-streaming-bound (512x512 filters x 36 = 38 MB for 64
    // rows) and F(2x2, 3x3) (16 positions, 4/9) is faster.  Measured per layer at 512x512, transforms included:
    // 256->256 at 64x64 42.4 -> 37.3 us, 512->256 at 64x64 67.4 -> 56.2; 512->512 at 32x32 38.3 -> 41.0 (kept on F(2x2)).
    // RIB_WINO_M = 2 / 4 forces one of them.
    const int wm = a.aux ? shortcut_wino_m(c, *a.aux, opname, Hout, Wout) : (pol.wino_force == 2 || pol.wino_force == 4 ? pol.wino_force : default_wino_m(Hout, Wout));
    const int NP = (wm + 2) * (wm + 2);      // output tile edge, Winograd positions
    const int tilesY = (Hout + wm - 1) / wm, tilesX = (Wout + wm - 1) / wm, ntiles = tilesY * tilesX;
    const std::string gname = opname + (wm == 2 ? ".wino" : ".wino4");
    // a fused 1x1 shortcut: K2 more columns in every row of V and U, written / read at the centre-tap positions only (kmask)
    const int K2 = a.aux ? a.aux->cinp : 0, ldv = c.cinp + K2;
    unsigned long long kmask = 0;
    if (a.aux) {
      if (a.aux_in.Cp != K2 || a.aux_in.H != Hout || a.aux_in.W != Wout || a.in.H != Hout || a.in.W != Wout) { error = opname + ": fused shortcut operand does not fit"; return false; }
      for (int r = 1; r <= wm; ++r) for (int q = 1; q <= wm; ++q) kmask |= 1ull << (r * (wm + 2) + q);
    }
    const size_t v_off = alloc((size_t)B * NP * ntiles * ldv * sizeof(float));
    const size_t m_off = alloc((size_t)B * NP * ntiles * c.coutp * sizeof(float));
    {   // input transform (with the convolution's prologue)
      OpOf<WinoInParams> op(RIB_KC_CONVAUX, opname + ".wino_in"); op.for_op = gname; op.wino_m = wm;
      WinoInParams& wi = op.p();
      wi.H = a.in.H; wi.W = a.in.W; wi.xC = a.in.Cp; wi.Cin = c.cinp; wi.tilesY = tilesY; wi.tilesX = tilesX;
      wi.pro_lrelu = a.pro_lrelu ? 1 : 0; wi.ldv = ldv;
      op.bind(&WinoInParams::x, WS(a.in.off)); op.bind(&WinoInParams::v, WS(v_off));
      if (a.in.lazy) {
        const LazySrc& L = *a.in.lazy;
        if (a.pro || a.pro_lrelu) { error = gname + ": a lazy input carries its own prologue"; return false; }
        op.wi_mode = L.mode;
        op.bind(&WinoInParams::x, WS(L.x.off)); wi.xC = L.x.Cp;
        wi.pro_ld = L.nx.ld;
        bind_norm(op, L.nx, gname, &WinoInParams::st, &WinoInParams::pro_scale, &WinoInParams::pro_shift);
        if (L.mode == WSRC_SPADE) {
          wi.x_ups = L.x_ups ? 1 : 0; wi.pro_lrelu = L.lrelu ? 1 : 0;
          op.bind(&WinoInParams::slab, WS(L.slab_off)); wi.slab_ld = L.slab_ld; wi.col0 = L.col0; op.bind(&WinoInParams::sbias, WT(L.sbias_off));
        } else {
          if (L.has2) {
            op.bind(&WinoInParams::x2, WS(L.x2.off));
            if (L.n2.ld != L.nx.ld) { error = gname + ": join operands with different statistics rows"; return false; }
            bind_norm(op, L.n2, gname, &WinoInParams::st2, &WinoInParams::pro2_scale, &WinoInParams::pro2_shift);
          } else op.bind(&WinoInParams::xres, WS(L.xres.off));
          op.bind(&WinoInParams::o, WS(L.o.off));
        }
      } else if (a.pro && !bind_norm(op, *a.pro, gname, &WinoInParams::st, &WinoInParams::pro_scale, &WinoInParams::pro_shift, a.pro_choff == 0, a.pro_choff)) {
        wi.pro_ld = a.pro->ld;      // (the row length of the arrays: unused with partials)
      }
      if (a.aux) {      // second source: the shortcut's input, stored or the never-stored second set of the block's first SPADE
        if (op.wi_mode == WSRC_JOIN) { error = gname + ": a join cannot carry a second source"; return false; }
        wi.nslices2 = (K2 + 63) / 64; wi.Cin2 = K2; wi.xC2 = a.aux_in.Cp;
        op.wi_mode2 = WSRC_PLAIN;
        if (a.aux_in.lazy) {
          const LazySrc& L = *a.aux_in.lazy;
          if (L.mode != WSRC_SPADE) { error = gname + ": lazy shortcut input of an unknown kind"; return false; }
          op.wi_mode2 = WSRC_SPADE;
          op.bind(&WinoInParams::x2, WS(L.x.off)); wi.xC2 = L.x.Cp; wi.pro2_ld = L.nx.ld; wi.x2_ups = L.x_ups ? 1 : 0; wi.lrelu2 = L.lrelu ? 1 : 0;
          bind_norm(op, L.nx, gname, &WinoInParams::st2, &WinoInParams::pro2_scale, &WinoInParams::pro2_shift);
          op.bind(&WinoInParams::slab2, WS(L.slab_off)); wi.slab2_ld = L.slab_ld; wi.col0_2 = L.col0; op.bind(&WinoInParams::sbias2, WT(L.sbias_off));
        } else op.bind(&WinoInParams::x2, WS(a.aux_in.off));
      }
      // workgroup = (16 (tile, transformed row) units per pass) x (slice of 64 channels)
      const int nsl = (c.cinp + 63) / 64 + wi.nslices2, units = ntiles * (wm + 2);
      // (every workgroup that reduces partials re-reads tiles x 64 channels x 16 bytes: few, fatter workgroups then)
      wi.nslices = nsl; wi.ublocks = std::max(1, std::min((units + 15) / 16, (wi.st.tiles > 0 ? 512 : 4096) / nsl));
      // Staged (k_wino_in_staged): workgroup = (block of sty x stx whole tiles, patch in LDS) x (slice of 64 channels).  The
      // largest block of the list wins whose grid still has a workgroup per CU, or as many as the unstaged grid where that
      // one has fewer (a fatter block fetches fewer halo pixels twice: 100 / 64 for 10 x 10 against 36 / 16 for 6 x 6).
      // The launch stays unstaged when (a) the staged kernel's static LDS would leave fewer than 2 workgroups per CU - it is
      // sized for the largest patch of the list, so this holds for every block or for none - or (b) no block of the list
      // keeps the grid at that bar.  Every class (tile x first source) of the 512x512 frame is faster staged
      // (profiles/r10_wino_in_staged.txt), so none is excluded here.
      if (h->wino_in_staging) {
        static const int kBlocks2[][2] = {{4, 4}, {2, 4}, {2, 2}}, kBlocks4[][2] = {{2, 2}, {1, 2}, {1, 1}};
        const int need = std::min((int)(wi.ublocks * nsl * B), 256 /* CUs */);
        const bool fits = 2 * WINO_STAGE_LDS_BYTES <= 160 * 1024 /* LDS of a CU */;
        for (int i = 0; i < 3 && fits && !op.wi_staged; ++i) {
          const int sty = std::min((wm == 4 ? kBlocks4 : kBlocks2)[i][0], tilesY), stx = std::min((wm == 4 ? kBlocks4 : kBlocks2)[i][1], tilesX);
          const int nblocks = ((tilesY + sty - 1) / sty) * ((tilesX + stx - 1) / stx);
          if ((wm * sty + 2) * (wm * stx + 2) > WINO_STAGE_MAX_PX || nblocks * nsl * B < need) continue;
          op.wi_staged = true; wi.sty = sty; wi.stx = stx; wi.ublocks = nblocks;
        }
      }
      op.grid = dim3(wi.ublocks * nsl, B, 1);
      push(op);
    }
    {   // the 16 / 36 GEMMs as one 1x1 "convolution" of NP*B samples of a tilesY x tilesX image, one filter set per position
      // k_gemm_dma (operands staged by LDS-DMA) unless a tuned choice names a k_igemm 1x1 variant; TB_() decides as for every choice
      Choice ch;
      ch.v = pick_gemm_dma(h->prec(), (long)TB_() * NP, ntiles, c.coutp, c.cinp);
      if (!ch.v) ch = choose_variant(h->prec(), 1, 1, false, false, c.coutp, TB_() * NP, tilesY, tilesX, c.cinp, false, 0, false);
      if (!tuned_choice({gname}, gname, "layer", &ch, [&](const Variant& tv, int ts) {
            return plain_1x1(tv, c.cinp) && ts == 1 && (!a.aux || tv.dma());
          })) return false;
      const Variant* v = ch.v;
      if (!v) { error = gname + ": no 1x1 kernel variant"; return false; }
      if (a.aux && !v->dma()) { error = gname + ": the fused shortcut needs a k_gemm_dma tile"; return false; }
      const int set = ensure_wino_set(h, (int)(&c - h->convs.data()), wm, a.aux ? (int)(a.aux - h->convs.data()) : -1);
      if (set < 0) { error = gname + ": " + h->err; return false; }
      // the convolution's algorithmic count (executed: 4/9 or 1/4 of it) + the shortcut's (executed as it is)
      const double fl = conv_flops(c, Hout, Wout, B) + (a.aux ? conv_flops(*a.aux, Hout, Wout, B) : 0.0);
      P->flops[RIB_KC_IGEMM] += fl;
      // M[n*NP + xi] = V[n*NP + xi] . U[xi]^T: Z = B*NP problems of ntiles x coutp x cinp (the zero bias: k_igemm form only)
      Gemm1x1 m;
      m.a = WS(v_off); m.w = WINO(set); m.c = WS(m_off); m.bias = WT(c.zero_off);
      m.Z = B * NP; m.H = tilesY; m.W = tilesX; m.K = c.cinp; m.N = c.coutp; m.lda = ldv; m.nsets = NP; m.K2 = K2; m.kmask = kmask;
      Op op = gemm_1x1(RIB_KC_IGEMM, gname, v, m, fl);
      op.wino = true; op.wino_m = wm;
      push(op);
    }
    {   // output transform + the convolution's epilogue
      OpOf<WinoOutParams> op(RIB_KC_CONVAUX, opname + ".wino_out"); op.for_op = gname; op.wino_m = wm;
      WinoOutParams& wo = op.p();
      // workgroup = (16 (tile, output row) units per pass) x (slice of 64 channels); ONE statistics partial per unit block,
      // at most STATS_MAX_PARTIALS of them, so the consumer of the normalised tensor can reduce them itself
      const int nsl = (c.coutp + 63) / 64, units = ntiles * wm;
      const int blocks = std::max(1, std::min((units + 15) / 16, (int)STATS_MAX_PARTIALS));
      wo.tilesY = tilesY; wo.tilesX = tilesX; wo.CoutPad = c.coutp; wo.ublocks = blocks; wo.nslices = nsl;
      wo.yC = a.out.Cp; wo.yoff = a.yoff; wo.Cout = stored_cout(a, c);
      wo.Hout = Hout; wo.Wout = Wout; wo.act = a.act;
      if (!out_fits(a, opname, Hout, Wout)) return false;
      op.bind(&WinoOutParams::m, WS(m_off)); op.bind(&WinoOutParams::bias, WT(a.aux ? c.fb_off : c.b_off)); op.bind(&WinoOutParams::y, WS(a.out.off));
      if (a.res) { op.bind(&WinoOutParams::res, WS(a.res->off)); wo.resC = a.res->Cp; }
      size_t part_off = 0;
      if (a.want_stats) { part_off = alloc_partials(B, blocks, c.coutp); op.bind(&WinoOutParams::stat_part, WS(part_off)); }
      op.grid = dim3(blocks * nsl, B, 1);
      push(op);
      if (a.want_stats) emit_stats(opname, a, part_off, blocks, Hout, Wout, B);
    }
    return true;
  }

  // ---- gamma/beta of EVERY SPADE of a condition level in one 1x1 GEMM (round 3) -----------------------------------------
  // The gamma/beta of a SPADE depend only on the condition map.  On the small deep maps (<= 64x64 at 512x512, batch 1) each
  // SPADE's own GEMM is a 10-30 us launch of which 10-13 us are ramp and drain, and the ten of them
  // that ran unfused were ten such launches.  The filter matrices of a level's SPADE groups lie back to back in the blob,
  // so ONE k_igemm 1x1 launch on cond[level] with N = sum of their columns (8192 at level 4, 2048 at level 3 of HSM.yaml:
  // 8.6 GFLOP each) writes a slab [B][H*W][N] and every SPADE of the level is then only its k_spade_modulate on its own
  // column range.  Levels whose map is larger stay fused (gamma/beta never touch memory there).
  bool cond_level_gemm(int level, const Act& cond) {
    const auto it = h->level_groups.find(level);
    if (it == h->level_groups.end() || it->second.size() < 2 || (long)TB_() * cond.H * cond.W > pol.cond_gemm_max_px) return true;      // (0: off)
    int N = 0; double fl = 0.0;
    for (int gi : it->second) {
      const SpadeGroup& sg = h->spades[gi];
      if (sg.col0 != N || h->padc(sg.cond) != cond.Cp) { error = fmt("cond level %d: SPADE group %s does not continue the level's filter matrix", level, sg.key.c_str()); return false; }
      N += sg.npad;
      fl += spade_flops(sg, cond.H, cond.W);
    }
    const SpadeGroup& first = h->spades[it->second[0]];
    const std::string name = fmt("cond_%d.gammabeta", level);
    Choice ch;
    ch.v = pick_gemm_dma(h->prec(), TB_(), cond.H * cond.W, N, cond.Cp);
    if (!ch.v) ch = choose_variant(h->prec(), 1, 1, false, false, N, TB_(), cond.H, cond.W, cond.Cp, false);
    if (!tuned_choice({name}, name, "launch", &ch, [&](const Variant& tv, int ts) { return plain_1x1(tv, cond.Cp) && ts == 1; })) return false;
    const Variant* v = ch.v;
    if (!v) { error = name + ": no 1x1 kernel variant"; return false; }
    const size_t slab_off = alloc((size_t)B * cond.H * cond.W * N * sizeof(float));
    P->flops[RIB_KC_SPADE] += fl;
    level_slab[level] = LevelSlab{slab_off, N};
    // slab[b] = cond[b] . W_level^T: B problems of (H*W) x N x Cp
    push(gemm_1x1(RIB_KC_SPADE, name, v, slab_gemm(cond, first, N, slab_off), fl));
    return true;
  }
  // the gamma/beta GEMM of SPADE group sg (or of the whole level that begins with it) on the condition map: N columns into a slab
  Gemm1x1 slab_gemm(const Act& cond, const SpadeGroup& sg, int N, size_t slab_off, int ksplit = 1) const {
    Gemm1x1 m;
    m.a = WS(cond.off); m.w = WT(h->mc16() ? sg.w16_off : sg.w_off); m.bias = WT(sg.b_off); m.c = WS(slab_off);
    m.Z = B; m.H = cond.H; m.W = cond.W; m.K = cond.Cp; m.N = N; m.lda = cond.Cp; m.ksplit = ksplit;
    return m;
  }
  // a tuned variant that can run a plain 1x1 GEMM with K input channels (either form)
  bool plain_1x1(const Variant& tv, int K) const {
    return tv.BF16 == h->prec() && tv.KS == 1 && tv.STRIDE == 1 && !tv.UPS && !tv.SPADE && tv.NF != 0 && K % tv.BK == 0;
  }

  // ---- SPADE launch: ys0 (= lrelu(mod0(x))), optional ys1 (= mods(x), no activation) -------
  // lazy_ok: the only consumer of ys0 is a convolution that runs in the Winograd domain - when this SPADE is just a modulate
  // of the level's gamma/beta slab, ys0 is not stored: the convolution's input transform computes it (LazySrc).
  // lazy1_ok: the same for ys1, the second set (the input of the learned shortcut, consumed by conv_block_1's input transform
  // as its second source).  A set whose consumer needs it stored is produced by k_spade_modulate, for that set alone.
  bool spade(const std::string& key, const Act& cond, const Act& x, bool x_ups, const Norm& nx,
             Act* ys0, Act* ys1, bool act0, bool lazy_ok = false, bool lazy1_ok = false) {
    const SpadeGroup& sg = h->spades[h->spade_index.at(key)];
    const int Hout = x_ups ? x.H * 2 : x.H, Wout = x_ups ? x.W * 2 : x.W;
    if (cond.H != Hout || cond.W != Wout) { error = fmt("%s: cond map %dx%d != %dx%d (SPADE resize must be the identity)", key.c_str(), cond.H, cond.W, Hout, Wout); return false; }
    if (cond.Cp != h->padc(sg.cond) || cond.Cp % 32 != 0) { error = fmt("%s: cond channels %d unsupported (need a multiple of 32)", key.c_str(), cond.Cp); return false; }
    if (x.Cp != sg.Cp) { error = fmt("%s: x channels %d != %d", key.c_str(), x.Cp, sg.Cp); return false; }
    // Fused (one kernel: gamma/beta GEMM + modulate epilogue) where the map is large; UNFUSED on the
    // small deep maps, where the fused kernel is one long K chain on a handful of workgroups: the
    // GEMM runs as a split-K 1x1 convolution into partial slabs and k_spade_modulate finishes.
    const Variant* v = choose_variant(h->prec(), 1, 1, false, true, sg.npad, TB_(), Hout, Wout, cond.Cp, false).v;
    if (sg.w1_off)      // 16 modulated channels: the one-fragment layout halves the matrix work (first fitting NF = 1 variant)
      for (int i = 0; i < kNumVariants; ++i) {
        const Variant& t = kVariants[i];
        if (t.SPADE && t.NF == 1 && t.BF16 == h->prec() && t.KW == 1 && t.TB == 1 && cond.Cp % t.BK == 0) { v = &t; break; }
      }
    Choice uf;   // unfused candidate
    const bool small_map = (long)Hout * Wout * TB_() <= 4096 && pol.unfused_spade;
    if (small_map) uf = choose_variant(h->prec(), 1, 1, false, false, sg.npad, TB_(), Hout, Wout, cond.Cp, true);
    bool unfused = small_map && uf.v != nullptr;
    Choice tc;      // a tuned entry names the fused kernel (a SPADE variant) or the GEMM of the unfused pair (a 1x1 convolution variant)
    if (!tuned_choice({key + ".spade"}, key, "layer", &tc, [&](const Variant& tv, int ts) {
          return !(tv.dma() || tv.BF16 != h->prec() || tv.KS != 1 || tv.STRIDE != 1 || tv.UPS || cond.Cp % tv.BK != 0 || ts < 1 || ts > cond.Cp / tv.BK || (tv.SPADE && ts != 1) ||
                   (tv.SPADE && tv.NF == 1 && !sg.w1_off));
        })) { error = key + ": tuned SPADE choice does not fit"; return false; }      // (this site's own wording)
    if (tc.v && tc.v->SPADE) { v = tc.v; unfused = false; }
    else if (tc.v) { uf = tc; unfused = true; }
    // the level's gamma/beta GEMM already ran (cond_level_gemm): this SPADE is only its modulate
    const auto lvl = level_slab.find(sg.level);
    const bool from_level = lvl != level_slab.end();
    if (from_level) unfused = true;
    if (!unfused && !v) { error = "no SPADE variant"; return false; }
    // sets that are never stored; set 1 lies (Cp / 32) gamma/beta column groups of 64 behind set 0, in the slab and in the bias
    const bool can_lazy = from_level && !h->keep_taps && pol.lazy_sources && h->prec() == PREC_F32;
    // (set 0 of a two-set SPADE only together with set 1: where conv_block_1 keeps its direct launch the plan stays as it was)
    const bool lz1 = can_lazy && lazy1_ok && sg.nsets == 2 && sg.Cp % 32 == 0;
    const bool lz0 = can_lazy && lazy_ok && (sg.nsets == 1 || lz1);
    const int set1_col = sg.Cp / 32 * 64;
    for (int set = 0; set < 2; ++set) {
      if (!(set ? lz1 : lz0)) continue;
      auto L = std::make_shared<LazySrc>();
      L->mode = WSRC_SPADE; L->name = key + ".spade.modulate"; L->x = x; L->nx = nx; L->x_ups = x_ups; L->lrelu = set ? false : act0;
      L->slab_off = lvl->second.off; L->slab_ld = lvl->second.ld; L->col0 = sg.col0 + set * set1_col; L->sbias_off = sg.b_off + set * set1_col;
      Act y; y.C = sg.C; y.Cp = sg.Cp; y.H = Hout; y.W = Wout; y.lazy = L;
      *(set ? ys1 : ys0) = y;
    }
    if (lz0 && (lz1 || sg.nsets == 1)) return true;
    // the stored sets: both, or set 0 alone when only set 1 is lazy (a launch over the first set's columns)
    const int mnsets = lz1 ? 1 : sg.nsets;
    if (unfused) {
      *ys0 = act(sg.C, Hout, Wout);
      if (sg.nsets == 2 && !lz1) *ys1 = act(sg.C, Hout, Wout);
      int S = 1, slab_ld = 0, col0 = 0;
      size_t slab_off = 0;
      if (from_level) {
        slab_off = lvl->second.off; slab_ld = lvl->second.ld; col0 = sg.col0;
      } else {
        S = uf.ksplit;
        slab_off = alloc((size_t)S * B * Hout * Wout * sg.npad * sizeof(float)); slab_ld = sg.npad;
        const double fl = spade_flops(sg, Hout, Wout);      // (cond is Hout x Wout: checked above)
        P->flops[RIB_KC_SPADE] += fl;
        push(gemm_1x1(RIB_KC_SPADE, key + ".spade", uf.v, slab_gemm(cond, sg, sg.npad, slab_off, S), fl));
      }
      OpOf<ModulateParams> mo(RIB_KC_ELTWISE, key + ".spade.modulate");
      ModulateParams& mp = mo.p();
      mp.ksplit = S; mp.B = B; mp.slab_ld = slab_ld; mp.col0 = col0; mp.xmC = x.Cp; mp.xm_ups = x_ups ? 1 : 0;
      mp.m_ld = nx.ld; mp.C = sg.Cp; mp.nsets = mnsets; mp.act0 = act0 ? ACT_LRELU : ACT_NONE; mp.act1 = ACT_NONE;
      mp.Hout = Hout; mp.Wout = Wout;
      mo.bind(&ModulateParams::slab, WS(slab_off)); mo.bind(&ModulateParams::bias, WT(sg.b_off)); mo.bind(&ModulateParams::xm, WS(x.off));
      // a slice of 64 virtual channels lies inside one set when C is a multiple of 64: the modulate can then reduce the
      // producer's partials of its own channels
      bind_norm(mo, nx, key + ".spade", &ModulateParams::st, &ModulateParams::m_scale, &ModulateParams::m_shift,
                sg.Cp % 64 == 0 && has_plain_partials(nx, sg.Cp));
      mo.bind(&ModulateParams::ys0, WS(ys0->off)); if (mnsets == 2) mo.bind(&ModulateParams::ys1, WS(ys1->off));
      const int nsl = (mnsets * sg.Cp + 63) / 64;
      mp.nslices = nsl; mp.pblocks = std::max(1, std::min((Hout * Wout + 15) / 16, (mp.st.tiles > 0 ? 384 : 2048) / nsl));
      mo.grid = dim3(mp.pblocks * nsl, B, 1);
      push(mo);
      return true;
    }
    *ys0 = act(sg.C, Hout, Wout);
    if (sg.nsets == 2) *ys1 = act(sg.C, Hout, Wout);
    OpOf<IgemmParams> op(RIB_KC_SPADE, key + ".spade"); op.var = v;
    IgemmParams& p = op.p();
    const bool one_frag = v->NF == 1;      // [gamma(16) | beta(16)] layout
    const int ncols = one_frag ? 32 : sg.npad;
    igemm_geometry(p, v, cond.H, cond.W, cond.Cp, cond.Cp, ncols, Hout, Wout);
    p.xmC = x.Cp; p.xm_ups = x_ups ? 1 : 0; p.m_ld = nx.ld; p.C = sg.Cp; p.nsets = sg.nsets;
    p.act0 = act0 ? ACT_LRELU : ACT_NONE; p.act1 = ACT_NONE;
    op.bind(&IgemmParams::x, WS(cond.off)); op.bind(&IgemmParams::w, WT(h->mc16() ? sg.w16_off : sg.w_off)); op.bind(&IgemmParams::bias, WT(sg.b_off));
    if (one_frag) { op.bind(&IgemmParams::w, WT(sg.w1_off)); op.bind(&IgemmParams::bias, WT(sg.b1_off)); }
    op.bind(&IgemmParams::xm, WS(x.off));
    // consumer-side finalize in the SPADE epilogue: not bind_norm - IgemmParams carries these partials in fields of its own
    // (m_part / m_tiles / m_Cs / m_inv), not in a StatSrc
    if (has_plain_partials(nx, sg.Cp)) {
      const FinalizeParams& q = nx.pend->q();
      op.bind(&IgemmParams::m_part, nx.pend->fin.ref(&FinalizeParams::part)); p.m_tiles = q.tiles; p.m_Cs = q.Cs; p.m_inv = q.inv_count;
    } else {
      materialize(nx, key + ".spade");
      op.bind(&IgemmParams::m_scale, WS(nx.sc)); op.bind(&IgemmParams::m_shift, WS(nx.sh));
    }
    op.bind(&IgemmParams::ys0, WS(ys0->off)); if (sg.nsets == 2) op.bind(&IgemmParams::ys1, WS(ys1->off));
    op.grid = dim3(p.tilesX * p.tilesY, (ncols + v->BN() - 1) / v->BN(), B);
    op.flops = spade_flops(sg, Hout, Wout);
    P->flops[RIB_KC_SPADE] += op.flops;
    push(op);
    return true;
  }

  // ---- Res2dBlock 'NACNAC' (PGNR/models/layers/residual.py:129-151) -------------------------
  bool spade_block(const std::string& name, const Act& x, bool x_ups, const Norm& nx, const Act& cond,
                   Act* out, Norm* nout) {
    const ConvDef& c0 = conv_of(h, name + ".conv_block_0");
    const ConvDef& c1 = conv_of(h, name + ".conv_block_1");
    const bool learned = h->conv_index.count(name + ".conv_block_s") > 0;
    const int Hout = x_ups ? x.H * 2 : x.H, Wout = x_ups ? x.W * 2 : x.W;
    Act ys0, ys1;
    Act hbuf = act(c0.cout, Hout, Wout);
    Norm nh = norm(hbuf.Cp);
    // learned shortcut (residual.py:98-108): its 1x1 convolution on SPADE_s(x) is fused into conv_block_1's launch as extra
    // K chunks accumulating into the same output tile - of the direct kernel, or of the Winograd-domain GEMM (wino1 below)
    const bool fuse_s = learned && pol.fuse_shortcut;
    // conv_block_1 runs in the Winograd domain with an identity shortcut at the same resolution (the res blocks), or with a
    // fused learned shortcut where the tuned table says so (shortcut_wino_m); both SPADE outputs it consumes are then lazy
    bool wino1;
    { ConvArgs t; t.cd = &c1;
      if (fuse_s) t.aux = &conv_of(h, name + ".conv_block_s"); else { t.res = &x; t.res_ups = !learned && x_ups; }
      wino1 = runs_wino(t, Hout, Wout, name + ".conv_block_1"); }
    { ConvArgs a; a.cd = &c0; a.out = hbuf; a.want_stats = true; a.stats_out = &nh;
      if (!spade(name + ".0", cond, x, x_ups, nx, &ys0, &ys1, true, runs_wino(a, Hout, Wout), fuse_s && wino1)) return false;
      if (!ys0.lazy) tap(name + ".ys0", ys0);
      a.in = ys0;
      if (!conv(a, name + ".conv_block_0")) return false; }
    tap(name + ".h", hbuf);
    Act y1, dummy;
    if (!spade(name + ".1", cond, hbuf, false, nh, &y1, &dummy, true, (!learned || fuse_s) && wino1)) return false;
    if (!y1.lazy) tap(name + ".y1", y1);
    Act outs;
    if (learned && !fuse_s) {
      const ConvDef& cs = conv_of(h, name + ".conv_block_s");
      outs = act(cs.cout, Hout, Wout);
      ConvArgs a; a.cd = &cs; a.in = ys1; a.out = outs;
      if (!conv(a, name + ".conv_block_s")) return false;
    }
    *out = act(c1.cout, Hout, Wout);
    { ConvArgs a; a.cd = &c1; a.in = y1; a.out = *out;
      if (fuse_s) { a.aux = &conv_of(h, name + ".conv_block_s"); a.aux_in = ys1; }
      else a.res = learned ? &outs : &x;
      a.res_ups = !learned && x_ups;   // identity shortcut of an upsampled input: x_up[y][x] = x[y>>1][x>>1]
      if (nout) { *nout = norm(out->Cp); a.want_stats = true; a.stats_out = nout; }
      if (!conv(a, name + ".conv_block_1")) return false; }
    tap(name, *out);
    return true;
  }

  // one of the two stride-2 encoders of the mask network (generator.py:449-459); its last level
  // lands in half of the concatenated tensor and of the concatenated (scale, shift) arrays
  bool mask_branch(int b, const Act& input, const Act& CAT, const Norm& ncat, int chm) {
    const rib_config& c = h->g.c;
    const std::string m = "flow_network_temp";
    const char* branches[2] = {"down_lbl", "down_img"};
    Act cur = input; Norm ncur; bool have = false;
    for (int i = 0; i <= c.mask_down; ++i) {
      const ConvDef& cd = conv_of(h, m + "." + branches[b] + "." + std::to_string(i));
      const bool lastl = (i == c.mask_down);
      Act o = lastl ? CAT : act(cd.cout, i == 0 ? cur.H : cur.H / 2, i == 0 ? cur.W : cur.W / 2);
      Norm no = lastl ? ncat : norm(h->padc(cd.cout));
      ConvArgs a; a.cd = &cd; a.in = cur; a.out = o;
      if (have) { a.pro = &ncur; a.pro_lrelu = true; }
      if (i >= 1) {      // same kernel choice as the paired launch of this level (mask_branches_paired): bit-identical results
        a.no_split = true;
        a.choice_names = {m + ".down_pair." + std::to_string(i), m + ".down_img." + std::to_string(i)};
      }
      // the last level's (scale, shift) land in the shared arrays of the concatenated tensor: its finalize is emitted at
      // the producer (`no` is a local copy of ncat: a deferred finalize attached to it would be lost)
      if (lastl) { a.yoff = b * chm; a.stats_choff = (size_t)b * chm; a.stats_now = true; }
      a.want_stats = true; a.stats_out = &no; a.affine = true;
      if (!conv(a, cd.name)) return false;
      if (!lastl) tap(std::string("mask.") + (b == 0 ? "lbl_" : "img_") + std::to_string(i) + ".raw", o);
      cur = o; ncur = no; have = true;
    }
    return true;
  }

  // Both stride-2 encoders of the mask network, level by level (round 3): level i >= 1 of the label encoder and of the image
  // encoder are the same convolution on different tensors with different filters (32 -> 64 -> 128 -> 256 channels at
  // HSM.yaml's widths, 2.4 GFLOP each), ~35 us launches that cannot fill the chip one at a time: ONE launch computes both
  // (IgemmParams::pair).  Level 0 reads different inputs (22 / 9 channels): two launches into the two halves of a 2-image
  // buffer.  Batch 1 only; a chain keeps the encoders apart (its label encoder runs once per segment at batch T).
  bool mask_branches_paired(const Act& L, const Act& I9, const Act& CAT, const Norm& ncat, int chm) {
    const rib_config& c = h->g.c;
    const std::string m = "flow_network_temp";
    const Act* inputs[2] = {&L, &I9};
    const char* branches[2] = {"down_lbl", "down_img"};
    Act cur; Norm ncur;
    {
      const ConvDef& c0 = conv_of(h, m + ".down_lbl.0");
      cur = act_n(2, c0.cout, L.H, L.W); ncur = norm(h->padc(c0.cout), 2);
      const size_t img_bytes = (size_t)L.H * L.W * cur.Cp * h->esz();
      for (int b = 0; b < 2; ++b) {
        const ConvDef& cd = conv_of(h, m + "." + branches[b] + ".0");
        Act o = cur; o.off += b * img_bytes;                                   // image b of the pair buffer
        Norm no = ncur; no.sc += (size_t)b * ncur.ld * sizeof(float); no.sh += (size_t)b * ncur.ld * sizeof(float);
        ConvArgs a; a.cd = &cd; a.in = *inputs[b]; a.out = o; a.want_stats = true; a.stats_out = &no; a.affine = true; a.stats_now = true;
        if (!conv(a, cd.name)) return false;
        tap(std::string("mask.") + (b == 0 ? "lbl_0" : "img_0") + ".raw", o);
      }
    }
    for (int i = 1; i <= c.mask_down; ++i) {
      const ConvDef& cl = conv_of(h, m + ".down_lbl." + std::to_string(i));
      const ConvDef& ci = conv_of(h, m + ".down_img." + std::to_string(i));
      const bool lastl = (i == c.mask_down);
      Act o = lastl ? CAT : act_n(2, cl.cout, cur.H / 2, cur.W / 2);
      Norm no = lastl ? ncat : norm(h->padc(cl.cout), 2);
      ConvArgs a; a.cd = &cl; a.pair = &ci; a.in = cur; a.out = o; a.pro = &ncur; a.pro_lrelu = true;
      if (lastl) { a.pair_merge = true; a.pair_yoff = chm; }
      a.want_stats = true; a.stats_out = &no; a.affine = true; a.no_split = true;
      a.choice_names = {m + ".down_pair." + std::to_string(i), m + ".down_img." + std::to_string(i)};
      if (!conv(a, m + ".down_pair." + std::to_string(i))) return false;
      if (!lastl) {
        const size_t img_bytes = (size_t)o.H * o.W * o.Cp * h->esz();
        Act ol = o, oi = o; oi.off += img_bytes;
        tap("mask.lbl_" + std::to_string(i) + ".raw", ol);
        tap("mask.img_" + std::to_string(i) + ".raw", oi);
      }
      cur = o; ncur = no;
    }
    return true;
  }

  // every workspace reference of a launch
  template <typename F> static void for_each_pref(Op& op, F f) {
    for (int i = 0; i < op.nbinds; ++i) if (op.binds[i].ref.sp == PS_WS) f(op.binds[i].ref);
  }
  AllocRec* alloc_of(size_t voff) {
    // allocations are in increasing voff order
    size_t lo = 0, hi = allocs.size();
    while (lo + 1 < hi) { const size_t mid = (lo + hi) / 2; if (allocs[mid].voff <= voff) lo = mid; else hi = mid; }
    return (!allocs.empty() && voff >= allocs[lo].voff && voff < allocs[lo].voff + allocs[lo].bytes) ? &allocs[lo] : nullptr;
  }
  // Lifetime analysis + placement; rewrites every workspace reference of the plan.  The plan runs its launches in
  // order on one stream, so a buffer is live from the first to the last launch that names it; buffers written outside
  // the plan (the label-only results rib_chain gathers into their slots before it runs the frame) are live from the
  // start, tapped activations (debug) until the end.
  bool assign_physical() {
    const bool reuse = pol.ws_reuse && !P->labels_only;
    if (!reuse) { P->ws_bytes = ws; return true; }
    bool bad = false;
    for (size_t i = 0; i < P->ops.size(); ++i)
      for_each_pref(P->ops[i], [&](PRef& r) {
        AllocRec* a = alloc_of(r.off);
        if (!a) { bad = true; return; }
        a->first = std::min(a->first, (int)i); a->last = std::max(a->last, (int)i);
      });
    if (bad) { error = "workspace reference outside every allocation"; return false; }
    const LabelSlots& l = P->ls;
    for (size_t off : {l.x0, l.nx_sc, l.nx_sh, l.cat, l.ncat_sc, l.ncat_sh})
      if (AllocRec* a = alloc_of(off)) a->first = -1;
    if (h->keep_taps)
      for (const Tap& t : P->taps)
        if (AllocRec* a = alloc_of(t.off)) a->last = INT_MAX;
    // placement: largest first, each at the lowest offset where it does not meet a placed buffer with an overlapping lifetime
    std::vector<int> order;
    for (size_t i = 0; i < allocs.size(); ++i) if (allocs[i].last >= 0 || allocs[i].first == -1) order.push_back((int)i);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return allocs[a].bytes != allocs[b].bytes ? allocs[a].bytes > allocs[b].bytes : a < b; });
    std::vector<int> placed;
    size_t top = 0;
    for (int i : order) {
      AllocRec& a = allocs[i];
      std::vector<std::pair<size_t, size_t>> busy;     // physical ranges of the placed buffers alive together with a
      for (int j : placed) {
        const AllocRec& b = allocs[j];
        if (b.first <= a.last && a.first <= b.last) busy.push_back({b.phys, b.phys + b.bytes});
      }
      std::sort(busy.begin(), busy.end());
      size_t at = 0;
      for (auto& r : busy) { if (at + a.bytes <= r.first) break; at = std::max(at, r.second); }
      a.phys = at;
      top = std::max(top, at + a.bytes);
      placed.push_back(i);
    }
    auto remap = [&](size_t voff) { AllocRec* a = alloc_of(voff); return a ? a->phys + (voff - a->voff) : voff; };
    for (Op& op : P->ops) for_each_pref(op, [&](PRef& r) { r.off = remap(r.off); });
    LabelSlots& m = P->ls;
    m.x0 = remap(m.x0); m.nx_sc = remap(m.nx_sc); m.nx_sh = remap(m.nx_sh); m.cat = remap(m.cat); m.ncat_sc = remap(m.ncat_sc); m.ncat_sh = remap(m.ncat_sh);
    for (Tap& t : P->taps) t.off = remap(t.off);
    P->ws_virtual = ws;
    P->ws_bytes = top;
    return true;
  }

  void record_label_slots(const Act& x, const Norm& nx, const Act& CAT, const Norm& ncat) {
    LabelSlots& l = P->ls;
    l.x0 = x.off; l.x0_b = (size_t)B * x.H * x.W * x.Cp * h->esz();
    l.nx_sc = nx.sc; l.nx_sh = nx.sh; l.nx_b = (size_t)B * nx.ld * sizeof(float);
    l.cat = CAT.off; l.cat_b = (size_t)B * CAT.H * CAT.W * CAT.Cp * h->esz();
    l.ncat_sc = ncat.sc; l.ncat_sh = ncat.sh; l.ncat_b = (size_t)B * ncat.ld * sizeof(float);
  }

  // the label-only launches alone (for rib_chain's batched pre-pass): pack.label, the mask network's label branch,
  // down_first; same tensors, same launch arguments as in build()
  bool build_labels() {
    const Cfg& g = h->g;
    const rib_config& c = g.c;
    const int H = P->H, W = P->W;
    P->labels_only = true;
    defer_stats = false;
    const bool vL = lowc_serves({"down_first", "flow_network_temp.down_lbl.0"});
    Act L = vL ? virt(c.label_nc, H, W, U_LABEL, c.label_nc) : act(c.label_nc, H, W);
    if (!vL && L.Cp > 32) { error = "input channel counts above 32 are not supported by the pack kernel"; return false; }
    if (!vL) pack("pack.label", L, U_LABEL, c.label_nc);
    const int chm = g.mask_nf(c.mask_down);
    if (h->padc(chm) != chm) { error = "mask network width must be a multiple of 8 (16 with bf16 storage)"; return false; }
    Act CAT = act(2 * chm, H >> c.mask_down, W >> c.mask_down);
    Norm ncat = norm(CAT.Cp);
    if (!mask_branch(0, L, CAT, ncat, chm)) return false;
    const ConvDef& df = conv_of(h, "down_first");
    Act x = act(df.cout, H, W); Norm nx = norm(x.Cp);
    ConvArgs a; a.cd = &df; a.in = L; a.out = x; a.want_stats = true; a.stats_out = &nx;
    if (!conv(a, "down_first")) return false;
    record_label_slots(x, nx, CAT, ncat);
    return assign_physical();
  }

  // ---- the frame plan, sub-network by sub-network (Generator.forward, PGNR/models/generator.py:181-234) ------------------
  // Tensors that more than one sub-network touches.  The planners below run in the order of `build()`, which is the order
  // of the launches AND of the workspace allocations (assign_physical() shares bytes by lifetime afterwards).
  struct Frame {
    Act L;                    // label map [B,22,H,W]: virtual (the caller's tensor, read in place by k_conv_lowc) or packed NHWC
    Act Ein;                  // cat([img_fake, img_prev]) (generator.py:197): the embedder's input
    Act I9;                   // cat([img_prev, img_fake, img]) (generator.py:232): the mask network's image input
    std::vector<Act> cond;    // condition maps of the embedder, level 0 (full resolution) .. emb_down
    Act CAT; Norm ncat;       // the mask network's concatenated encoder outputs [label | image] and their InstanceNorm
    int chm = 0, Hm = 0, Wm = 0;
  };

  // boundary: NCHW user tensors -> NHWC (+concat, +zero channel padding), or nothing at all where k_conv_lowc reads them in place
  bool plan_boundary(Frame& F) {
    const rib_config& c = h->g.c;
    const int H = P->H, W = P->W;
    // Where the first layers can read the caller's NCHW tensors in place (k_conv_lowc) there is no packed copy at all
    const bool vL = lowc_serves({"down_first", "flow_network_temp.down_lbl.0"});
    const bool vE = lowc_serves({"ref_embedding.conv_first"});
    const bool vI = lowc_serves({"flow_network_temp.down_img.0"}) && head_without_nhwc(conv_of(h, "conv_img"));
    F.L = vL ? virt(c.label_nc, H, W, U_LABEL, c.label_nc) : act(c.label_nc, H, W);
    F.Ein = vE ? virt(c.image_nc * 2, H, W, U_FAKE, c.image_nc, U_PREV, c.image_nc) : act(c.image_nc * 2, H, W);     // cat([img_fake, img_prev]) generator.py:197
    F.I9 = vI ? virt(c.image_nc * 3, H, W, U_PREV, c.image_nc, U_FAKE, c.image_nc, U_IMG, c.image_nc) : act(c.image_nc * 3, H, W);   // cat([img_prev, img_fake, img]) generator.py:232
    if (F.L.Cp > 32 || F.Ein.Cp > 32 || F.I9.Cp > 32) { error = "input channel counts above 32 are not supported by the pack kernel"; return false; }   // (Cp = 0 for the unpacked ones)
    mark_label = true;
    if (!vL) pack("pack.label", F.L, U_LABEL, c.label_nc);
    mark_label = false;
    if (!vI) pack("pack.img9", F.I9, U_PREV, c.image_nc, U_FAKE, c.image_nc);           // cat([img_prev, img_fake, .]) generator.py:232
    if (!vE) pack("pack.embed_in", F.Ein, U_FAKE, c.image_nc, U_PREV, c.image_nc);      // cat([img_fake, img_prev]) generator.py:197
    return true;
  }

  // ref_embedding (LabelEmbedder 'encoder', generator.py:360-387) + gamma/beta of the SPADEs of the small condition levels
  bool plan_embedder(Frame& F) {
    const rib_config& c = h->g.c;
    const int H = P->H, W = P->W;
    std::vector<Act>& cond = F.cond;
    cond.assign(c.emb_down + 1, Act());
    {
      const ConvDef& cf = conv_of(h, "ref_embedding.conv_first");
      cond[0] = act(cf.cout, H, W);
      ConvArgs a; a.cd = &cf; a.in = F.Ein; a.out = cond[0]; a.act = ACT_LRELU;
      if (!conv(a, "ref_embedding.conv_first")) return false;
      tap("cond_0", cond[0]);
      for (int i = 0; i < c.emb_down; ++i) {
        const ConvDef& cd = conv_of(h, "ref_embedding.down_" + std::to_string(i));
        cond[i + 1] = act(cd.cout, cond[i].H / 2, cond[i].W / 2);
        ConvArgs b; b.cd = &cd; b.in = cond[i]; b.out = cond[i + 1]; b.act = ACT_LRELU;
        if (!conv(b, cd.name)) return false;
        tap("cond_" + std::to_string(i + 1), cond[i + 1]);
      }
    }
    // gamma/beta of all SPADEs of the small condition levels, one GEMM per level (cond_level_gemm)
    for (int j = 0; j <= c.emb_down; ++j)
      if (!cond_level_gemm(j, cond[j])) return false;
    return true;
  }

  // label encoder of the mask network: depends only on the label map, so a chain runs it once per segment (labels-only plan);
  // in a paired frame plan it rides with the image encoder instead (plan_mask_net)
  bool plan_mask_label_branch(Frame& F) {
    const Cfg& g = h->g;
    const rib_config& c = g.c;
    const int H = P->H, W = P->W;
    F.chm = g.mask_nf(c.mask_down);
    F.Hm = H >> c.mask_down; F.Wm = W >> c.mask_down;
    const int chm = F.chm;
    if (h->padc(chm) != chm) { error = "mask network width must be a multiple of 8 (16 with bf16 storage)"; return false; }
    F.CAT = act(2 * chm, F.Hm, F.Wm);
    F.ncat = norm(F.CAT.Cp);
    if (!pair_mask) {
      mark_label = true;
      if (!mask_branch(0, F.L, F.CAT, F.ncat, chm)) return false;
      mark_label = false;
    }
    return true;
  }

  // main generator (generator.py:201-228): down_first, down_0..D with AvgPool, res blocks, up_D..0, conv_img + tanh
  bool plan_trunk(Frame& F) {
    const Cfg& g = h->g;
    const rib_config& c = g.c;
    const int H = P->H, W = P->W;
    const int D = c.num_down_img;
    const std::vector<Act>& cond = F.cond;
    Act x; Norm nx;
    {
      const ConvDef& df = conv_of(h, "down_first");
      x = act(df.cout, H, W); nx = norm(x.Cp);
      ConvArgs a; a.cd = &df; a.in = F.L; a.out = x; a.want_stats = true; a.stats_out = &nx;
      mark_label = true;
      if (!conv(a, "down_first")) return false;
      mark_label = false;
      tap("down_first", x);
    }
    record_label_slots(x, nx, F.CAT, F.ncat);
    for (int i = 0; i <= D; ++i) {
      Act out; Norm nout;
      const bool last = (i == D);
      if (!spade_block("down_" + std::to_string(i), x, false, nx, cond[std::min(c.emb_down, i)], &out, last ? &nout : nullptr)) return false;
      if (!last) {   // self.downsample = AvgPool2d(3, 2, 1) (generator.py:127,207-208)
        if (out.Cp % 4 != 0 || 256 % (out.Cp / 4) != 0) { error = "avgpool: unsupported channel count"; return false; }
        Act pooled = act(out.C, out.H / 2, out.W / 2);
        Norm np = norm(pooled.Cp);
        const int slots = 256 / (out.Cp / 4), ppb = slots * 4;
        const int blocks = (pooled.H * pooled.W + ppb - 1) / ppb;
        const size_t part = alloc_partials(B, blocks, out.Cp);
        OpOf<PoolParams> op(RIB_KC_POOL, "down_" + std::to_string(i) + ".pool");
        op.p().H = out.H; op.p().W = out.W; op.p().C = out.Cp; op.p().blocks = blocks;
        op.bind(&PoolParams::x, WS(out.off)); op.bind(&PoolParams::y, WS(pooled.off)); op.bind(&PoolParams::stat_part, WS(part));
        op.grid = dim3(blocks, B, 1);
        push(op);
        // (not a convolution: no ConvArgs for emit_stats to read - the pool keeps its own two lines)
        finalize_or_defer(finalize_op(op.name, part, blocks, out.Cp, out.Cp, np, 0, pooled.H, pooled.W, nullptr, B), &np, false);
        x = pooled; nx = np;
      } else { x = out; nx = nout; }
    }
    const int jres = std::min(c.emb_down, D + 1);
    for (int i = 0; i < g.num_res_blocks(); ++i) {
      Act out; Norm nout;
      if (!spade_block("res_" + std::to_string(i), x, false, nx, cond[jres], &out, &nout)) return false;
      x = out; nx = nout;
    }
    bool ups = false;
    for (int i = D; i >= 0; --i) {
      Act out; Norm nout;
      // statistics of a nearest-x2 upsampled tensor equal those of the tensor itself, so the
      // producer's (scale, shift) are reused and the upsample is folded into the consumer's read
      if (!spade_block("up_" + std::to_string(i), x, ups, nx, cond[std::min(i, c.emb_down)], &out, i != 0 ? &nout : nullptr)) return false;
      x = out; nx = nout; ups = true;
    }
    {   // conv_img 'AC' + tanh (generator.py:114-116,228); also lands in img9[6:9]
      const ConvDef& ci = conv_of(h, "conv_img");
      ConvArgs a; a.cd = &ci; a.in = x; a.pro_lrelu = true; a.out = F.I9; a.yoff = c.image_nc * 2;
      a.cout_store = c.image_nc; a.act = ACT_TANH; a.y_nchw = US(U_IMG);
      a.y_none = F.I9.virt;      // the mask network then reads the image from the caller's NCHW tensor
      if (!conv(a, "conv_img")) return false;
    }
    return true;
  }

  // MaskGenerator (generator.py:493-510): image encoder (paired with the label encoder where the plan pairs), join with the
  // label branch, res_flow blocks, phase-convolution decoder, sigmoid head (+ the driver's blend)
  bool plan_mask_net(Frame& F) {
    const rib_config& c = h->g.c;
    const int H = P->H, W = P->W;
    const std::string m = "flow_network_temp";
    const int chm = F.chm, Hm = F.Hm, Wm = F.Wm;
    const Act& CAT = F.CAT; const Norm& ncat = F.ncat;
    if (pair_mask ? !mask_branches_paired(F.L, F.I9, CAT, ncat, chm) : !mask_branch(1, F.I9, CAT, ncat, chm)) return false;
    tap("mask.cat.raw", CAT);
    Act r; bool first = true;
    for (int i = 0; i < c.mask_res_blocks; ++i) {
      const std::string bn = m + ".res_flow." + std::to_string(i);
      const ConvDef& c0 = conv_of(h, bn + ".conv_block_0");
      const ConvDef& c1 = conv_of(h, bn + ".conv_block_1");
      const bool learned = h->conv_index.count(bn + ".conv_block_s") > 0;
      const Act xin = first ? CAT : r;                              // (lazy: the previous block's join, computed by this block's first input transform)
      const Act xin_stored = xin.lazy ? xin.lazy->o : xin;          // ... which also stores it: the residual of this block's join
      Act t0 = act(c0.cout, Hm, Wm); Norm n0 = norm(t0.Cp);
      { ConvArgs a; a.cd = &c0; a.in = xin; a.out = t0; if (first) { a.pro = &ncat; a.pro_lrelu = true; }
        a.want_stats = true; a.stats_out = &n0; a.affine = true;
        if (!conv(a, c0.name)) return false; }
      Act t1 = act(c1.cout, Hm, Wm); Norm n1 = norm(t1.Cp);
      { ConvArgs a; a.cd = &c1; a.in = t0; a.out = t1; a.pro = &n0; a.pro_lrelu = true;
        a.want_stats = true; a.stats_out = &n1; a.affine = true;
        if (!conv(a, c1.name)) return false; }
      Act ts; Norm ns;
      if (learned) {
        const ConvDef& cs = conv_of(h, bn + ".conv_block_s");
        ts = act(cs.cout, Hm, Wm); ns = norm(ts.Cp);
        ConvArgs a; a.cd = &cs; a.in = xin; a.out = ts; if (first) { a.pro = &ncat; a.pro_lrelu = true; }
        a.want_stats = true; a.stats_out = &ns; a.affine = true;
        if (!conv(a, cs.name)) return false;
      } else if (first) { error = "mask res block 0 must have a learned shortcut"; return false; }
      Act o = act(c1.cout, Hm, Wm);
      {
        // the join feeds the next block's conv_block_0 (no prologue): when that runs in the Winograd domain its input
        // transform computes the join on the fly and stores it
        ConvArgs t;
        if (i + 1 < c.mask_res_blocks) t.cd = &conv_of(h, m + ".res_flow." + std::to_string(i + 1) + ".conv_block_0");
        if (t.cd && pol.lazy_sources && h->prec() == PREC_F32 && runs_wino(t, Hm, Wm) && t.cd->cinp == o.Cp && n1.ld == o.Cp) {
          auto L = std::make_shared<LazySrc>();
          L->mode = WSRC_JOIN; L->name = bn + ".join"; L->x = t1; L->nx = n1; L->o = o;
          if (learned) { L->has2 = true; L->x2 = ts; L->n2 = ns; } else L->xres = xin_stored;
          Act y = o; y.lazy = L;
          tap("mask.res_" + std::to_string(i), o);
          r = y; first = false;
          continue;
        }
      }
      OpOf<InAddParams> op(RIB_KC_ELTWISE, bn + ".join");
      InAddParams& ap = op.p();
      ap.C = o.Cp; ap.HW = Hm * Wm; ap.ld = n1.ld;
      op.bind(&InAddParams::t1, WS(t1.off));
      bind_norm(op, n1, std::string(), &InAddParams::st1, &InAddParams::sc1, &InAddParams::sh1);
      if (learned) {
        op.bind(&InAddParams::ts, WS(ts.off));
        bind_norm(op, ns, std::string(), &InAddParams::sts, &InAddParams::scs, &InAddParams::shs);
      } else op.bind(&InAddParams::xres, WS(xin_stored.off));
      op.bind(&InAddParams::out, WS(o.off));
      const int nsl = (o.Cp + 63) / 64;
      ap.nslices = nsl; ap.pblocks = std::max(1, std::min((Hm * Wm + 15) / 16, ((ap.st1.tiles > 0 || ap.sts.tiles > 0) ? 384 : 2048) / nsl));
      op.grid = dim3(ap.pblocks * nsl, B, 1);
      push(op);
      tap("mask.res_" + std::to_string(i), o);
      r = o; first = false;
    }
    Act cur = r; Norm ncur; bool have = false;
    for (int j = 0; j < c.mask_down; ++j) {
      const ConvDef& cd = conv_of(h, m + ".up_flow." + std::to_string(2 * j + 1));
      Act o = act(cd.cout, cur.H * 2, cur.W * 2); Norm no = norm(o.Cp);
      ConvArgs a; a.cd = &cd; a.in = cur; a.ups = true; a.out = o;
      if (have) { a.pro = &ncur; a.pro_lrelu = true; }
      a.want_stats = true; a.stats_out = &no; a.affine = true;
      if (!conv(a, cd.name)) return false;
      tap("mask.up_" + std::to_string(j) + ".raw", o);
      cur = o; ncur = no; have = true;
    }
    {
      const ConvDef& cm = conv_of(h, m + ".conv_mask.0");
      ConvArgs a; a.cd = &cm; a.in = cur; if (have) { a.pro = &ncur; a.pro_lrelu = true; }
      a.act = ACT_SIGMOID; a.y_user = US(U_MASK);
      if (!conv(a, cm.name)) return false;
    }
    return true;
  }

  bool build() {
    Frame F;
    return plan_boundary(F) && plan_embedder(F) && plan_mask_label_branch(F) && plan_trunk(F) && plan_mask_net(F) && assign_physical();
  }
};

}  // namespace
