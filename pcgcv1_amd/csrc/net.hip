// Whole-transform executors behind pcgc_net_* (include/pcgc.h).
//
// Layer tables restate models/model_voxception.py (AnalysisTransform 71-144,
// SynthesisTransform 147-214, HyperEncoder 217-252, HyperDecoder 255-308,
// _VoxceptionResNet 11-68); they must match pcgcv1_amd/models/spec.py, which the
// Python host uses to order the parameter list.
//
// The reference runs one cube per call (tf.map_fn, transform.py:116-147, 224-257);
// here a batch is cut into chunks of cubes small enough that the chunk's working
// set stays in the 256 MiB Infinity Cache and large enough to fill 256 CUs, and
// every layer is one launch over the whole chunk.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"

namespace pcgc {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

struct LayerDef {
  const char* name;
  int tconv, cin, cout, k, stride, bias, relu;
};

static void push_vrn(std::vector<LayerDef>& L, int c) {
  const int q = c / 4, h = c / 2;
  L.push_back({"conv1_1", 0, c, q, 3, 1, 1, 1});
  L.push_back({"conv1_2", 0, q, h, 3, 1, 1, 1});
  L.push_back({"conv2_1", 0, c, q, 1, 1, 1, 1});
  L.push_back({"conv2_2", 0, q, q, 3, 1, 1, 1});
  L.push_back({"conv2_3", 0, q, h, 1, 1, 1, 1});
}

static std::vector<LayerDef> layer_table(int kind) {
  std::vector<LayerDef> L;
  switch (kind) {
    case PCGC_NET_ANALYSIS:
      L.push_back({"conv_in", 0, 1, 16, 3, 1, 1, 1});
      for (int i = 0; i < 3; ++i) push_vrn(L, 16);
      L.push_back({"down_1", 0, 16, 32, 3, 2, 0, 1});
      for (int i = 0; i < 3; ++i) push_vrn(L, 32);
      L.push_back({"down_2", 0, 32, 64, 3, 2, 0, 1});
      for (int i = 0; i < 3; ++i) push_vrn(L, 64);
      L.push_back({"conv_out", 0, 64, 16, 3, 1, 1, 0});
      break;
    case PCGC_NET_SYNTHESIS:
      L.push_back({"deconv_in", 0, 16, 64, 3, 1, 1, 1});
      for (int i = 0; i < 3; ++i) push_vrn(L, 64);
      L.push_back({"up_1", 1, 64, 32, 3, 2, 1, 1});
      for (int i = 0; i < 3; ++i) push_vrn(L, 32);
      L.push_back({"up_2", 1, 32, 16, 3, 2, 1, 1});
      for (int i = 0; i < 3; ++i) push_vrn(L, 16);
      L.push_back({"deconv_out", 0, 16, 1, 3, 1, 1, 0});
      break;
    case PCGC_NET_HYPER_ENCODER:
      L.push_back({"conv1", 0, 16, 16, 3, 1, 1, 1});
      L.push_back({"conv2", 0, 16, 16, 3, 2, 1, 1});
      L.push_back({"conv3", 0, 16, 8, 3, 1, 1, 0});
      break;
    case PCGC_NET_HYPER_DECODER:
      L.push_back({"conv1", 0, 8, 16, 3, 1, 1, 1});
      L.push_back({"conv2", 1, 16, 16, 3, 2, 1, 1});
      L.push_back({"conv3", 0, 16, 32, 3, 1, 1, 1});
      L.push_back({"conv4_1", 0, 32, 16, 3, 1, 1, 0});
      L.push_back({"conv4_2", 0, 32, 16, 3, 1, 1, 0});
      break;
    default:
      break;
  }
  return L;
}

// Layer indices of the two autoencoder transforms (both: in, three blocks, resample, three blocks, resample, three blocks,
// out); pcgc_net_create checks them against layer_table()
enum { kLayerIn = 0, kLayerVrn1 = 1, kLayerResample1 = 16, kLayerVrn2 = 17, kLayerResample2 = 32, kLayerVrn3 = 33, kLayerOut = 48 };
static bool layer_indices_match(const std::vector<LayerDef>& L) {
  bool ok = L.size() == kLayerOut + 1 && L[kLayerResample1].stride == 2 && L[kLayerResample2].stride == 2;
  for (int l : {kLayerVrn1, kLayerVrn2, kLayerVrn3}) ok = ok && !strcmp(L[l].name, "conv1_1") && !strcmp(L[l + 14].name, "conv2_3");
  return ok;
}

struct LayerW {
  LayerDef def;
  const float* w_tf;    // device, TF layout
  const float* bias;    // device or nullptr
  const float* w_mfma;  // device, packed (nullptr when no MFMA kernel takes this shape at any size)
  const float* w_row = nullptr;   // device, LDS image of the row kernel that takes this layer (up_2, down_1), or nullptr
};

// the ten pointers (kernel, bias of conv1_1, conv1_2, conv2_1, conv2_2, conv2_3) the block kernels take; l = index of conv1_1
struct BlockW { const float* p[10]; };
static BlockW block_weights(const std::vector<LayerW>& Ls, size_t l) {
  BlockW w;
  for (int i = 0; i < 5; ++i) { w.p[2 * i] = Ls[l + i].w_tf; w.p[2 * i + 1] = Ls[l + i].bias; }
  return w;
}

// which kernel took a launch (pcgc_net_profile_report prints the name)
enum Kern { K_DIRECT, K_MFMA, K_KS, K_KS1, K_KS2, K_VRN_A, K_VRN_BC, K_VALU, K_ROW_A, K_ROW_BC, K_ROW_IN, K_ROW_OUT, K_ROW_B, K_ROW_C,
            K_ROW_UP, K_ROW_DOWN, K_ROW_H8, K_ROW_HUP, K_ROW_HDOWN, K_SEG_A, K_SEG_BC, K_SEG_IN, K_COUNT };
static const char* const kKernName[K_COUNT] = {"direct", "mfma", "ks", "ks1", "ks2", "vrnA", "vrnBC", "valu", "rowA", "rowBC", "rowin", "rowout",
                                               "rowB", "rowC", "rowup", "rowdown", "rowh8", "rowhup", "rowhdown", "segA", "segBC", "segin"};

}  // namespace pcgc

struct ProfRec { int layer, kern, B, Din; hipEvent_t t0, t1; };

struct pcgc_net {
  int kind, algo, chunk;   // algo: 0 auto, 1 direct only; chunk: cubes per chunk asked for at creation (0: the defaults)
  std::vector<pcgc::LayerW> layers;
  float* blob = nullptr;   // all weights (TF + packed), library-owned device memory
  // analysis only: the 64^3 and the 32^3 stage's responses to an EMPTY cube (RowSkip, common.h), one cube each, laid out as
  // kEmpty (net_plan.h); library-owned like the weights.  E64 / E32 = the blob once that stage's responses are in it
  float* empty_blob = nullptr;
  const float *E64 = nullptr, *E32 = nullptr;
  const pcgc::TileCfg* skip_cfg = nullptr;  // device table of the kSkipLaunches launch geometries of the 64^3 stage (in empty_blob)
  const pcgc::TileCfg* skip_cfg_mid[2] = {nullptr, nullptr};   // ... of the 32^3 stage's six launches: [0] large launches, [1] <= 16 cubes
  unsigned* skip_counter = nullptr;   // tests: device word that counts the wave tiles skipped (pcgc_net_set_skip_counter)
  bool profiling = false; mutable std::vector<ProfRec> prof;
};

namespace pcgc {

static inline int mode_of(const LayerDef& d) { return d.tconv ? 2 : (d.stride == 2 ? 1 : 0); }

struct Exec {
  const pcgc_net* net; hipStream_t s; int B;  // B: cubes in this chunk

  ConvArgs args(const LayerW& L, const float* x, int Din, int x_cs, int x_co, float* y, int y_cs, int y_co,
                const float* res, int absval = 0, float lb = 0.f) const {
    ConvArgs a;
    a.x = x; a.w = L.w_tf; a.bias = L.bias; a.y = y; a.res = res;
    a.B = B; a.Din = Din;
    a.Dout = L.def.tconv ? Din * 2 : Din / L.def.stride;
    a.Cin = L.def.cin; a.Cout = L.def.cout;
    a.x_cs = x_cs; a.x_co = x_co; a.y_cs = y_cs; a.y_co = y_co;
    a.ksize = L.def.k; a.mode = mode_of(L.def); a.relu = L.def.relu;
    a.absval = absval; a.lower_bound = lb;
    a.w2 = nullptr; a.bias2 = nullptr; a.y2 = nullptr; a.y2_cs = 0; a.cout2 = 0;
    return a;
  }

  // launch(kern) runs between two profiling events; it sets kern to the kernel that took the launch.  Profiling is an aid,
  // not part of the data path: a launch whose events cannot be created / recorded is simply not listed
  template <class F>
  int timed(int layer, int D, F&& launch) const {
    ProfRec pr{layer, K_DIRECT, B, D, nullptr, nullptr};
    const bool on = net->profiling && hipEventCreate(&pr.t0) == hipSuccess && hipEventCreate(&pr.t1) == hipSuccess &&
                    hipEventRecord(pr.t0, s) == hipSuccess;
    const int rc = launch(pr.kern);
    if (on && hipEventRecord(pr.t1, s) == hipSuccess) net->prof.push_back(pr);
    return rc;
  }

  // launch one (possibly fused) layer; fuse as in launch_conv_ks
  int run(const LayerW& L, const ConvArgs& a, int fuse) const {
    if (fuse && (net->algo == 1 || !L.w_mfma)) { set_error("fused launch requested on the direct path"); return -1; }
    return timed((int)(&L - net->layers.data()), a.Din, [&](int& kern) {
      int rc = 0;
      if (net->algo != 1 && fuse == 0 && (L.def.cin == 1 || L.def.cout == 1) && (rc = launch_conv_valu(a, s, true)) != 0) {
        if (rc > 0) { kern = K_VALU; rc = 0; }     // conv_in / deconv_out: LDS-tiled VALU kernel
      } else if (net->algo != 1 && L.w_mfma) {
        rc = launch_conv_ks(a, L.w_mfma, fuse, s, true);
        if (rc > 0) { kern = K_KS + fuse; rc = 0; }
        else if (rc == 0 && fuse == 0) {
          rc = launch_conv_mfma(a, L.w_mfma, s, true);
          if (rc > 0) { kern = K_MFMA; rc = 0; } else if (rc == 0) rc = launch_conv_direct(a, s);
        } else if (rc == 0) {
          set_error("fused VRN kernel unavailable for a shape it was planned for");
          rc = -1;
        }
      } else {
        rc = launch_conv_direct(a, s);
      }
      return rc;
    });
  }

  int conv(const LayerW& L, const float* x, int Din, int x_cs, int x_co, float* y, int y_cs, int y_co,
           const float* res, int absval = 0, float lb = 0.f, int x_q4 = 0, int y_q4 = 0) const {
    ConvArgs a = args(L, x, Din, x_cs, x_co, y, y_cs, y_co, res, absval, lb);
    a.x_q4 = x_q4; a.y_q4 = y_q4;
    return run(L, a, 0);
  }

  // one launch of a kernel that has no other form (the row kernels of vrn_row.hip, ...)
  template <class F>
  int row(int layer, int kern, int D, F&& launch) const {
    return timed(layer, D, [&](int& k) { k = kern; return launch(); });
  }

  // _VoxceptionResNet.call (model_voxception.py:56-68); l = index of conv1_1. x -> out, both [B,D^3,C].
  // q4: x / out are Q4 tensors (the 64^3 stage of the transforms): the row kernels of vrn_row.hip
  // x_nonneg: x is the output of a ReLU (the layer before the stage, or the previous block)
  int vrn(int l, const float* x, float* out, int D, int C, float* t1, float* t2, float* t3, bool q4 = false, bool x_nonneg = false,
          const RowSkip* skipA = nullptr, const RowSkip* skipBC = nullptr) const {
    const auto& Ls = net->layers;
    const int q = C / 4, h = C / 2;
    int rc;
    if (q4) {
      const bool big = C == 16 && D == 64, mid = C == 32 && D == 32, low = C == 64 && D == 16;
      if (!big && !mid && !low) { set_error("Q4 VRN block needs C=16 at D=64, C=32 at D=32 or C=64 at D=16 (got C=%d D=%d)", C, D); return -1; }
      const BlockW w = block_weights(Ls, l);
      static const int kern_low[3] = {K_ROW_A, K_ROW_B, K_ROW_C}, kern_2[2] = {K_ROW_A, K_ROW_BC};
      for (int which = 0; which < (low ? 3 : 2); ++which)       // C = 64: A, B, C (vrn_row16.hip); else A, BC
        if ((rc = row(l + which, low ? kern_low[which] : kern_2[which], D, [&] {
               return big ? launch_vrn16_row(x, t1, out, w.p, B, which, s, x_nonneg, which == 0 ? skipA : skipBC)
                          : (mid ? launch_vrn32_row(x, t1, out, w.p, B, which, s, x_nonneg, which == 0 ? skipA : skipBC, Ls[l].w_row)
                                 : launch_vrn64_row(x, t1, out, w.p, B, which, s, Ls[l].w_row)); })))
          return rc;
      return 0;
    }
    if (net->algo != 1 && C == 16 && D % 16 == 0) {
      // full-resolution blocks: two VALU kernels (vrn_valu.hip)
      const BlockW w = block_weights(Ls, l);
      for (int which = 0; which < 2; ++which) {
        rc = row(l + which, K_VRN_A + which, D, [&] { return launch_vrn16_valu(x, t1, out, w.p, B, D, which, s); });
        if (rc <= 0) { if (rc == 0) set_error("vrn16 VALU kernel refused D=%d", D); return rc < 0 ? rc : -1; }
      }
      return 0;
    }
    if (net->algo != 1 && Ls[l].w_mfma && Ls[l + 2].w_mfma && Ls[l + 3].w_mfma) {
      // fused form: [conv1_1 + conv2_1] -> conv1_2(+residual) -> [conv2_2 + conv2_3 + residual]
      ConvArgs a1 = args(Ls[l + 0], x, D, C, 0, t1, q, 0, nullptr);
      a1.w2 = Ls[l + 2].w_mfma; a1.bias2 = Ls[l + 2].bias; a1.y2 = t2; a1.y2_cs = q; a1.cout2 = q;
      ConvArgs a3 = args(Ls[l + 3], t2, D, q, 0, out, C, h, x);
      a3.w2 = Ls[l + 4].w_tf; a3.bias2 = Ls[l + 4].bias; a3.cout2 = h;
      if (launch_conv_ks(a1, Ls[l].w_mfma, 1, s, false) == 1 && launch_conv_ks(a3, Ls[l + 3].w_mfma, 2, s, false) == 1) {
        if ((rc = run(Ls[l + 0], a1, 1))) return rc;
        if ((rc = conv(Ls[l + 1], t1, D, q, 0, out, C, 0, x))) return rc;
        return run(Ls[l + 3], a3, 2);
      }
    }
    if ((rc = conv(Ls[l + 0], x, D, C, 0, t1, q, 0, nullptr))) return rc;         // tensor1_1
    if ((rc = conv(Ls[l + 2], x, D, C, 0, t2, q, 0, nullptr))) return rc;         // tensor2_1
    if ((rc = conv(Ls[l + 1], t1, D, q, 0, out, C, 0, x))) return rc;             // relu(x[:h] + tensor1_2)
    if ((rc = conv(Ls[l + 3], t2, D, q, 0, t3, q, 0, nullptr))) return rc;        // tensor2_2
    if ((rc = conv(Ls[l + 4], t3, D, q, 0, out, C, h, x))) return rc;             // relu(x[h:] + tensor2_3)
    return 0;
  }
};

// Scheduling of a batch.  The three resolutions of the auto-encoder transforms want different chunk
// sizes: at 64^3 a chunk of a few cubes already gives thousands of workgroups and its activations
// (25 MB / cube with the blocks running in place) should stay inside the 256 MiB Infinity Cache; at 16^3 a cube is only 16 workgroups, so
// ~128 cubes are needed to fill 256 CUs.  A "super chunk" of cubes therefore runs stage by stage, the
// stage boundaries (down_k / up_k outputs) being kept for the whole super chunk.  Where everything lies in the
// caller's workspace is the NetPlan's business (net_plan.h): the same plan sizes and carves it.
constexpr size_t kSegWindowPad = 2u << 20;      // bytes: the window starts this far below the chunk's tensors (SegArgs)

// The plan of one call.  The experiment knobs are read here, once per CALL: tests compare the settings in one process.
static NetPlan make_plan(const pcgc_net* net, int B, int D) {
  auto env_int = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
  Chunks asked{0, 0, 0};
  int a = 0, b = 0, d = 0;
  const char* env = getenv(net->kind == PCGC_NET_ANALYSIS ? "PCGC_CHUNKS_A" : "PCGC_CHUNKS_S");   // experiment knobs
  if (!env) env = getenv("PCGC_CHUNKS");            // "big,mid,small" cubes per launch at D, D/2, D/4
  if (env && sscanf(env, "%d,%d,%d", &a, &b, &d) == 3 && a > 0 && b > 0 && d > 0) asked = Chunks{a, b, d};
  if (net->chunk > 0) asked = Chunks{net->chunk, net->chunk, net->chunk};
  NetPlan p = plan_net(net->kind, B, D, asked, env_int("PCGC_SKIP_EMPTY", 3), net->E64 != nullptr);
  p.skip_mid = env_int("PCGC_SKIP_MID", 1) != 0; p.copy_empty = env_int("PCGC_SEG_COPY_EMPTY", 0) != 0;
  return p;
}
template <class T>
static T* region(char* ws, const NetPlan& p, Region r) { return reinterpret_cast<T*>(ws + p.r[r].at); }

// empty-space skipping in a stage's three blocks (RowSkip): the chunk's tables in the workspace `ws`, the responses e + at->...
struct StageSkip {
  const char* ws;
  ChunkView v;
  const float* e;
  const StageOffsets* at;
  bool virtual_tiles;       // 64^3 stage: empty tiles are not written, readers get the `virt` tables
  bool unread_ok;           // ... and down_1 skips its own empty tiles
  RowSkip launch(int c, size_t e_off, unsigned* counter) const {      // launch c of the chunk; e_off = its own response in the layout
    RowSkip r;
    r.order = v.order.in(ws, c); r.n_heavy = v.n_heavy.in(ws, c); r.empty = e + e_off; r.counter = counter;
    return r;
  }
};

// three VRN blocks starting at layer l, IN PLACE on `a`: every kernel that writes the block output reads the block
// input only for the residual, at the very element it then overwrites (vrn16_bc, the `res` epilogues), and the
// kernels that read the input with a halo (conv1_1 / conv2_1) run before any of those.  One activation tensor
// instead of two keeps a 64^3 chunk's working set (x + t12 = 201 MB for 8 cubes) inside the 256 MiB Infinity
// Cache, where the ping-pong pair (250 MB at 6 cubes) thrashed it (measured: vrn16_bc 14.6 -> 13.0 ms per step).
static int vrn3(const Exec& E, int l, float* a, int d, int c, float* t, size_t full, bool q4 = false, const StageSkip* k = nullptr) {
  for (int i = 0; i < 3; ++i) {
    // block 0 follows layer l - 1 (conv_in / down_* / deconv_in / up_*: ReLU per the layer table), the others a block
    const bool nonneg = i > 0 || (l > 0 && E.net->layers[l - 1].def.relu);
    RowSkip ka, kbc;
    if (k) {
      const int cA = k->v.A0 + 2 * i, cBC = cA + 1;
      const float *e_t = k->e + k->at->t[i], *e_prev = k->e + (i == 0 ? k->at->first : k->at->o[i - 1]);
      ka = k->launch(cA, k->at->t[i], E.net->skip_counter);
      kbc = k->launch(cBC, k->at->o[i], E.net->skip_counter);
      if (k->virtual_tiles) {
        // virtual tiles (64^3 stage): A reads the block input, made by the launch before it (conv_in or the previous block's
        // BC); BC reads A's output with its halo and the block input as residual.  The stage's last launch copies its empty
        // tiles for down_1 — all, or (down_1 skipping its own empty tiles: `unread_ok`) only those a computed down_1 tile reads
        ka.materialize = 0; ka.in_virtual = k->v.virt.in(k->ws, cA - 1); ka.in_empty = e_prev;
        kbc.materialize = i == 2 ? (k->unread_ok ? 2 : 1) : 0;
        kbc.in_virtual = k->v.virt.in(k->ws, cA); kbc.in_empty = e_t;
        kbc.res_virtual = ka.in_virtual; kbc.res_empty = e_prev;
      }
    }
    int rc = E.vrn(l + 5 * i, a, a, d, c, t, t + full / 4, t + full / 2, q4, nonneg, k ? &ka : nullptr, k ? &kbc : nullptr);
    if (rc) return rc;
  }
  return 0;
}

// The three C = 16 blocks of the analysis' 64^3 stage on slots (vrn_seg.hip), in place on `a`: per block kernel A reads the block
// input (conv_in's output or the previous block's, slots not written there = the producer's empty-cube response) and writes
// tensor1_1 | tensor2_1 for its heavy slots, kernel BC reads those with their halo and the block input as residual.  `win` =
// the window's base; k.e = the responses INSIDE the window.  down_1 reads the stage's output through the last launch's table.
static int vrn3_seg(const Exec& E, int l0, float* a, float* t, const char* win, const StageSkip& k) {
  const auto& Ls = E.net->layers;
  const int max_slots = E.B * (int)kSlots;
  auto off = [&](const void* p) { return (unsigned)((const char*)p - win); };
  for (int i = 0; i < 3; ++i) {
    const int l = l0 + 5 * i, cA = k.v.A0 + 2 * i, cBC = cA + 1;
    const bool nonneg = i > 0 || (l > 0 && Ls[l - 1].def.relu);
    SegArgs sa;
    sa.win = win; sa.x_off = off(a); sa.t_off = off(t); sa.out_off = off(a);
    sa.w11 = Ls[l].w_tf; sa.b11 = Ls[l].bias; sa.w12 = Ls[l + 1].w_tf; sa.b12 = Ls[l + 1].bias; sa.w21 = Ls[l + 2].w_tf; sa.b21 = Ls[l + 2].bias;
    sa.w22 = Ls[l + 3].w_tf; sa.b22 = Ls[l + 3].bias; sa.w23 = Ls[l + 4].w_tf; sa.b23 = Ls[l + 4].bias;
    sa.slots = k.v.slots.in(k.ws, cA); sa.n_slots = k.v.counts.in(k.ws, cA);
    sa.in_virt = k.v.seg_virt.in(k.ws, cA - 1); sa.ein_off = off(k.e + (i == 0 ? k.at->first : k.at->o[i - 1]));
    int rc = E.row(l, K_SEG_A, 64, [&] { return launch_vrn16_seg(sa, 0, nonneg, max_slots, E.s); });
    if (rc) return rc;
    sa.slots = k.v.slots.in(k.ws, cBC); sa.n_slots = k.v.counts.in(k.ws, cBC);
    sa.res_virt = sa.in_virt; sa.eres_off = sa.ein_off;
    sa.in_virt = k.v.seg_virt.in(k.ws, cA); sa.ein_off = off(k.e + k.at->t[i]);
    if ((rc = E.row(l + 1, K_SEG_BC, 64, [&] { return launch_vrn16_seg(sa, 1, nonneg, max_slots, E.s); }))) return rc;
  }
  return 0;
}

static int forward_autoencoder(const pcgc_net* net, const NetPlan& p, const float* x, float* out, int B, int D, char* ws, size_t ws_bytes,
                               hipStream_t s) {
  PCGC_REQUIRE(p.total <= ws_bytes, "pcgc_net_forward: the plan needs %zu bytes of workspace behind the aligned base, %zu given", p.total, ws_bytes);
  const bool ana = net->kind == PCGC_NET_ANALYSIS;
  const auto& Ls = net->layers;
  const LayerW &Lin = Ls[kLayerIn], &Lr1 = Ls[kLayerResample1], &Lr2 = Ls[kLayerResample2], &Lout = Ls[kLayerOut];
  const int Db = ana ? D : 4 * D, Dm = Db / 2, Ds = Db / 4, SC = p.SC;
  const size_t V = p.V, s2_cube = p.s2_cube, s3_cube = p.s3_cube; const Chunks ch = p.ch;
  float *S2 = region<float>(ws, p, R_S2), *S3 = region<float>(ws, p, R_S3), *work = region<float>(ws, p, R_WORK);
  // the full-resolution stage runs on the row kernels (vrn_row.hip) with its activations in the Q4 layout
  static const int stages = getenv("PCGC_ROW_STAGES") ? atoi(getenv("PCGC_ROW_STAGES")) : 127;   // experiment knob: bit per stage
  const bool q4 = net->algo != 1 && Db == 64 && (stages & 1);
  const bool q4m = net->algo != 1 && Dm == 32 && (stages & 2);     // the middle stage (C = 32 at 32^3) likewise: vrn_row32.hip
  const bool q4s = net->algo != 1 && Ds == 16 && (stages & 4);     // and the low-resolution stage (C = 64 at 16^3): vrn_row16.hip
  // exact skipping of empty space in the analysis' 64^3 stage (RowSkip): PCGC_SKIP_EMPTY=0 computes every tile.  Its tables
  // are filled once per super chunk (three launches), before the stages.
  const bool skip = ana && q4 && p.mode != 0 && p.responses;
  unsigned long long* rowocc = region<unsigned long long>(ws, p, R_ROWOCC);
  // the blocks on slots (PCGC_SKIP_EMPTY=3): one buffer window of < 2 GiB holds the chunk's tensors and the responses
  const bool seg = skip && p.mode == 3 && q4m && (stages & 16) && Lr1.w_row;     // (down_1's row kernel reads the slot-wise output)
  const char* win = nullptr;
  const float* e64 = net->E64;                                 // the 64^3 stage's responses the kernels read: e64 + kEmpty.s64...
  if (seg) {
    // Where the net's blob itself lies within reach of the chunk's tensors — one window of < 2 GiB covers both — the kernels
    // read the responses in place; else (or with PCGC_SEG_COPY_EMPTY=1) they are copied behind the scratch, 92 MB per call
    const size_t e_bytes = kEmpty.copy_floats() * sizeof(float);
    float* ec = region<float>(ws, p, R_EMPTY_COPY);
    const char* lo = reinterpret_cast<const char*>(work);
    const char* hi = reinterpret_cast<const char*>(ec);          // everything of the chunk lies below the copy's place
    const char* blob_lo = reinterpret_cast<const char*>(net->E64 + kEmpty.s64.first);
    const char* wlo = blob_lo < lo ? blob_lo : lo;
    const char* whi = blob_lo + e_bytes > hi ? blob_lo + e_bytes : hi;
    if (!p.copy_empty && (size_t)(whi - wlo) + kSegWindowPad < 0x7ffff000u) {
      win = wlo - kSegWindowPad;
    } else {
      PCGC_CHECK_HIP(hipMemcpyAsync(ec, blob_lo, e_bytes, hipMemcpyDeviceToDevice, s));
      win = lo - kSegWindowPad;
      e64 = ec - kEmpty.s64.first;
    }
    PCGC_REQUIRE((size_t)(reinterpret_cast<const char*>(e64 + kEmpty.s64.end) - win) < 0x7ffff000u &&
                 (size_t)(ws + p.r[R_SEG_VIRT].at - win) < 0x7ffff000u,
                 "analysis: the 64^3 chunk and the empty-cube responses do not fit one 2 GiB buffer window");
  }
  const bool virtual_tiles = skip && (p.mode == 1 || p.mode == 3);
  // ... and in down_1 + the 32^3 stage (copy mode: every tile stays materialised); PCGC_SKIP_MID=0 stops at the 64^3 stage
  const bool skip_mid = skip && q4m && (stages & 16) && Lr1.w_row && net->E32 && p.skip_mid;
  int rc;
  for (int b0 = 0; b0 < B; b0 += SC) {
    const int nb = std::min(SC, B - b0);
    const int big = equal_chunk(nb, ch.big);
    if (ana) {
      if (skip) {                                              // row occupancy and every chunk's tile orders: they depend on the input only
        if (seg) {
          unsigned long long* occ64 = region<unsigned long long>(ws, p, R_OCC64);
          if ((rc = launch_voxocc(x + (size_t)b0 * V, occ64, rowocc, nb, s))) return rc;
          if ((rc = launch_seg_order(occ64, rowocc, nb, big, region<unsigned>(ws, p, R_SEG_SLOTS), region<unsigned>(ws, p, R_SEG_COUNTS),
                                     region<unsigned char>(ws, p, R_SEG_VIRT), net->skip_counter, s))) return rc;
        } else if ((rc = launch_rowocc(x + (size_t)b0 * V, rowocc, nb, s))) return rc;
        if ((rc = launch_tile_order(rowocc, nb, big, net->skip_cfg, nullptr, kSkipLaunches, region<unsigned>(ws, p, R_ORDER),
                                    region<unsigned>(ws, p, R_N_HEAVY), (int)kTiles64, region<unsigned long long>(ws, p, R_VIRT), s))) return rc;
        if (skip_mid && (rc = launch_tile_order(rowocc, nb, ch.mid, net->skip_cfg_mid[0], net->skip_cfg_mid[1], kSkipLaunchesMid,
                                                region<unsigned>(ws, p, R_ORDER_MID), region<unsigned>(ws, p, R_N_HEAVY_MID), (int)kTiles32, nullptr, s))) return rc;
      }
      // 64^3: conv_in, vrn1_*, down_1 -> S2
      for (int c0 = 0; c0 < nb; c0 += big) {
        const int n = std::min(big, nb - c0);
        Exec E{net, s, n};
        const size_t full = (size_t)n * V * 16;
        float* A = work; float* t = A + full;
        const float* xin = x + (size_t)(b0 + c0) * V;
        const StageSkip sk{ws, p.chunk64(c0, n, c0 / big), e64, &kEmpty.s64, virtual_tiles, skip_mid};
        if (seg) {                                             // conv_in on slots
          ConvInSegArgs ca;
          ca.x = xin; ca.win = win; ca.out_off = (unsigned)((const char*)A - win);
          ca.slots = sk.v.slots.in(ws, l64::conv_in); ca.n_slots = sk.v.counts.in(ws, l64::conv_in);
          ca.w = Lin.w_tf; ca.bias = Lin.bias; ca.relu = Lin.def.relu;
          rc = E.row(kLayerIn, K_SEG_IN, Db, [&] { return launch_conv_in_seg(ca, n * (int)kSlots, s); });
        } else if (q4) {
          RowSkip kin = sk.launch(l64::conv_in, kEmpty.s64.first, net->skip_counter);
          kin.materialize = virtual_tiles ? 0 : 1;
          rc = E.row(kLayerIn, K_ROW_IN, Db, [&] { return launch_conv_in_row(xin, A, Lin.w_tf, Lin.bias, n, Lin.def.relu, s, skip ? &kin : nullptr); });
        } else rc = E.conv(Lin, xin, Db, 1, 0, A, 16, 0, nullptr);
        if (rc) return rc;
        if ((rc = seg ? vrn3_seg(E, kLayerVrn1, A, t, win, sk) : vrn3(E, kLayerVrn1, A, Db, 16, t, full, q4, skip ? &sk : nullptr))) return rc;
        float* down_out = S2 + (size_t)c0 * s2_cube;
        RowSkip kd1 = sk.launch(l64::down_1, 0, net->skip_counter);      // down_1: the last of the chunk's tile orders, copy mode
        kd1.empty = skip_mid ? net->E32 + kEmpty.s32.first : nullptr;
        SegRead sr;                                            // the blocks ran on slots: down_1 reads their output through the last launch's table
        if (seg) {
          sr.win = win; sr.x_off = (unsigned)((const char*)A - win); sr.e_off = (unsigned)((const char*)(e64 + kEmpty.s64.o[2]) - win);
          sr.virt = sk.v.seg_virt.in(ws, l64::BC(2));
        }
        if (q4 && q4m && (stages & 16) && Lr1.w_row) {
          rc = E.row(kLayerResample1, K_ROW_DOWN, Db, [&] {
            return launch_down1_row(A, down_out, Lr1.w_row, Lr1.bias, n, Lr1.def.relu, s, skip_mid ? &kd1 : nullptr, false, nullptr, seg ? &sr : nullptr); });
        }
        else if (seg) { set_error("analysis: the segment form of the 64^3 blocks needs down_1's row kernel"); return -1; }
        else rc = E.conv(Lr1, A, Db, 16, 0, down_out, 32, 0, nullptr, 0, 0.f, q4, q4m);
        if (rc) return rc;
      }
      // 32^3: vrn2_*, down_2 -> S3
      for (int c0 = 0; c0 < nb; c0 += ch.mid) {
        const int n = std::min(ch.mid, nb - c0);
        Exec E{net, s, n};
        float* r = S2 + (size_t)c0 * s2_cube;         // the blocks run in place on the stage buffer
        // this chunk's six tile orders (made for the tiles launch_vrn32_row uses at this launch size)
        const StageSkip sk{ws, p.chunk32(c0, n, c0 / ch.mid), net->E32, &kEmpty.s32, false, false};
        if ((rc = vrn3(E, kLayerVrn2, r, Dm, 32, work, (size_t)n * s2_cube, q4m, skip_mid ? &sk : nullptr))) return rc;
        float* down2_out = S3 + (size_t)c0 * s3_cube;
        if (q4m && q4s && (stages & 64) && Lr2.w_row) rc = E.row(kLayerResample2, K_ROW_DOWN, Dm, [&] { return launch_down2_row(r, down2_out, Lr2.w_row, Lr2.bias, n, Lr2.def.relu, s); });
        else rc = E.conv(Lr2, r, Dm, 32, 0, down2_out, 64, 0, nullptr, 0, 0.f, q4m, q4s);
        if (rc) return rc;
      }
      // 16^3: vrn3_*, conv_out
      for (int c0 = 0; c0 < nb; c0 += ch.small) {
        const int n = std::min(ch.small, nb - c0);
        Exec E{net, s, n};
        float* r = S3 + (size_t)c0 * s3_cube;         // the blocks run in place on the stage buffer
        if ((rc = vrn3(E, kLayerVrn3, r, Ds, 64, work, (size_t)n * s3_cube, q4s))) return rc;
        if ((rc = E.conv(Lout, r, Ds, 64, 0, out + (size_t)(b0 + c0) * (V / 64) * 16, 16, 0, nullptr, 0, 0.f, q4s, 0))) return rc;
      }
    } else {
      // 16^3: deconv_in, vrn1_*, up_1 -> S2
      for (int c0 = 0; c0 < nb; c0 += ch.small) {
        const int n = std::min(ch.small, nb - c0);
        Exec E{net, s, n};
        const size_t full = (size_t)n * (V / 64) * 64;
        float* A = work; float* t = A + full;
        if ((rc = E.conv(Lin, x + (size_t)(b0 + c0) * (V / 64) * 16, Ds, 16, 0, A, 64, 0, nullptr, 0, 0.f, 0, q4s))) return rc;
        if ((rc = vrn3(E, kLayerVrn1, A, Ds, 64, t, full, q4s))) return rc;
        float* up1_out = S2 + (size_t)c0 * s2_cube;
        if (q4s && q4m && (stages & 32) && Lr1.w_row) rc = E.row(kLayerResample1, K_ROW_UP, Ds, [&] { return launch_up1_row(A, up1_out, Lr1.w_row, Lr1.bias, n, Lr1.def.relu, s); });
        else rc = E.conv(Lr1, A, Ds, 64, 0, up1_out, 32, 0, nullptr, 0, 0.f, q4s, q4m);
        if (rc) return rc;
      }
      // 32^3: vrn2_* in place on S2
      for (int c0 = 0; c0 < nb; c0 += ch.mid) {
        const int n = std::min(ch.mid, nb - c0);
        Exec E{net, s, n};
        if ((rc = vrn3(E, kLayerVrn2, S2 + (size_t)c0 * s2_cube, Dm, 32, work, (size_t)n * s2_cube, q4m))) return rc;
      }
      // 64^3: up_2, vrn3_*, deconv_out per chunk — the 16-channel full-resolution tensor (16.8 MB per cube) never
      // makes the round trip through HBM: up_2 writes it chunk by chunk right before the blocks that consume it
      for (int c0 = 0; c0 < nb; c0 += big) {
        const int n = std::min(big, nb - c0);
        Exec E{net, s, n};
        const size_t full = (size_t)n * V * 16;
        float* A = work; float* t = A + full;
        const float* up_in = S2 + (size_t)c0 * s2_cube;
        if (q4 && q4m && (stages & 8) && Lr2.w_row) rc = E.row(kLayerResample2, K_ROW_UP, Dm, [&] { return launch_up2_row(up_in, A, Lr2.w_row, Lr2.bias, n, Lr2.def.relu, s); });
        else rc = E.conv(Lr2, up_in, Dm, 32, 0, A, 16, 0, nullptr, 0, 0.f, q4m, q4);
        if (rc) return rc;
        if ((rc = vrn3(E, kLayerVrn3, A, Db, 16, t, full, q4))) return rc;
        float* yout = out + (size_t)(b0 + c0) * V;
        if (q4) rc = E.row(kLayerOut, K_ROW_OUT, Db, [&] { return launch_deconv_out_row(A, yout, Lout.w_tf, Lout.bias, n, Lout.def.relu, s); });
        else rc = E.conv(Lout, A, Db, 16, 0, yout, 1, 0, nullptr);
        if (rc) return rc;
      }
    }
  }
  return 0;
}

// one chunk (<= kHyperChunk cubes) of the hyper encoder / decoder; f1 .. f3 = the plan's activation regions
static int forward_chunk(const pcgc_net* net, const float* x, float* out0, float* out1, int B, int D,
                         float lb, float* f1, float* f2, float* f3, hipStream_t s) {
  Exec E{net, s, B};
  const auto& Ls = net->layers;
  int rc;
  if (net->kind == PCGC_NET_HYPER_ENCODER) {
    if ((rc = E.conv(Ls[0], x, D, 16, 0, f1, 16, 0, nullptr))) return rc;
    if (net->algo != 1 && D == 16) rc = E.row(1, K_ROW_HDOWN, 16, [&] { return launch_down8_row(f1, f2, Ls[1].w_tf, Ls[1].bias, B, Ls[1].def.relu, s); });
    else rc = E.conv(Ls[1], f1, D, 16, 0, f2, 16, 0, nullptr);
    if (rc) return rc;
    if (net->algo != 1 && D / 2 == 8) {                   // 8^3: plane-vector row kernel (hyper_row.hip)
      rc = E.row(2, K_ROW_H8, 8, [&] { return launch_conv8_row(f2, out0, Ls[2].w_tf, Ls[2].bias, B, 16, 8, Ls[2].def.relu, s); });
      if (rc != 0) return rc < 0 ? rc : 0;
    }
    return E.conv(Ls[2], f2, D / 2, 16, 0, out0, 8, 0, nullptr);
  }
  if (net->kind == PCGC_NET_HYPER_DECODER) {
    if (net->algo != 1 && D == 8) {                       // 8^3 layers: plane-vector row kernels (hyper_row.hip)
      rc = E.row(0, K_ROW_H8, 8, [&] { return launch_conv8_row(x, f1, Ls[0].w_tf, Ls[0].bias, B, 8, 16, Ls[0].def.relu, s); });
      if (rc < 0) return rc;
      if (rc == 0) { set_error("hyper decoder conv1: no 8^3 row kernel for 8 -> 16"); return -1; }
      if ((rc = E.row(1, K_ROW_HUP, 8, [&] { return launch_up8_row(f1, f2, Ls[1].w_tf, Ls[1].bias, B, Ls[1].def.relu, s); }))) return rc;
    } else {
      if ((rc = E.conv(Ls[0], x, D, 8, 0, f1, 16, 0, nullptr))) return rc;
      if ((rc = E.conv(Ls[1], f1, D, 16, 0, f2, 16, 0, nullptr))) return rc;
    }
    if ((rc = E.conv(Ls[2], f2, 2 * D, 16, 0, f3, 32, 0, nullptr))) return rc;
    if ((rc = E.conv(Ls[3], f3, 2 * D, 32, 0, out0, 16, 0, nullptr))) return rc;
    return E.conv(Ls[4], f3, 2 * D, 32, 0, out1, 16, 0, nullptr, /*absval=*/1, lb);  // |scale| clamped
  }
  set_error("unknown net kind %d", net->kind);
  return -1;
}

// floats per cube of output `which` (the hyper decoder alone has a second one) and of the input
static size_t out_floats_per_cube(int kind, int D, int which) {
  const size_t d3 = (size_t)D * D * D, per[4] = {d3 / 64 * 16, d3 * 64, d3 / 8 * 8, d3 * 8 * 16};
  return kind >= 0 && kind < 4 && (which == 0 || kind == PCGC_NET_HYPER_DECODER) ? per[kind] : 0;
}
static size_t in_floats_per_cube(int kind, int D) {
  const size_t channels[4] = {1, 16, 16, 8};
  return kind >= 0 && kind < 4 ? (size_t)D * D * D * channels[kind] : 0;
}

}  // namespace pcgc

using namespace pcgc;

// The analysis' 64^3 and 32^3 stages applied to ONE all-zero cube, kept per layer output (RowSkip; EmptyLayout): the very
// kernels of the forward pass, every tile computed — so a skipped tile's copy is bit-identical to what the wave would have computed.
static int make_empty_responses(pcgc_net* net, hipStream_t s) {
  float* b = nullptr;
  PCGC_CHECK_HIP(hipMalloc(&b, kEmpty.total * sizeof(float)));
  net->empty_blob = b;
  // launch geometries (tile rows x planes: vrn_row.hip, vrn_row32.hip) and the fine (64^3) window each output depends on.
  // 64^3 stage: conv_in radius 1; block i: tensor1_1 2 + 2i (tensor2_1 less: it shares the launch), block output 3 + 2i.
  // down_1 (stride 2, nothing padded in front, one voxel behind): output o reads fine 2o .. 2o + 2 of a radius-7 tensor
  // = [2o - 7, 2o + 9]; every 3^3 layer at 32^3 adds two fine voxels on each side.
  TileCfg cfg[kSkipLaunches + 2 * kSkipLaunchesMid];
  cfg[l64::conv_in] = {2, 4, 1, 1, 1};
  for (int i = 0; i < 3; ++i) { cfg[l64::A(i)] = {2, 8, 2 + 2 * i, 2 + 2 * i, 1}; cfg[l64::BC(i)] = {2, 8, 3 + 2 * i, 3 + 2 * i, 1}; }
  // the stage's last launch: a down_1 tile (2 x 2 outputs at 32^3) reads fine rows / planes [2o, 2o + 4] and is computed
  // iff [2o - 7, 2o + 11] holds an occupied row, so an empty tile here is read only if its own rows / planes dilated by
  // 4 + 7 = 11 do (TileCfg::need)
  cfg[l64::BC(2)].need = 4 + 7;
  cfg[l64::down_1] = {kDown1TileRows, kDown1TilePlanes, 7, 9, 2};
  static_assert(kDown1TileRows == 2 && kDown1TilePlanes == 2, "the `need` radius above is derived for 2 x 2 down_1 tiles");
  for (int v = 0; v < 2; ++v)                                  // v = 0: launches of > 16 cubes, v = 1: small launches
    for (int i = 0; i < kSkipLaunchesMid; ++i) {               // i = l32::A(block) / l32::BC(block)
      int th, ld;
      vrn32_tile_geometry(v == 0 ? 64 : 1, i & 1, &th, &ld);
      cfg[kSkipLaunches + v * kSkipLaunchesMid + i] = TileCfg{th, ld, 9 + 2 * i, 11 + 2 * i, 2};
    }
  TileCfg* cfg_dev = reinterpret_cast<TileCfg*>(b + kEmpty.cfg);
  static_assert(sizeof(cfg) <= 256 * sizeof(float), "the configuration tables fit behind the tensors");
  PCGC_CHECK_HIP(hipMemcpyAsync(cfg_dev, cfg, sizeof(cfg), hipMemcpyHostToDevice, s));
  PCGC_CHECK_HIP(hipStreamSynchronize(s));                   // cfg lives on this stack frame
  net->skip_cfg = cfg_dev;
  net->skip_cfg_mid[0] = cfg_dev + kSkipLaunches;
  net->skip_cfg_mid[1] = cfg_dev + kSkipLaunches + kSkipLaunchesMid;
  const StageOffsets &e64 = kEmpty.s64, &e32 = kEmpty.s32;
  PCGC_CHECK_HIP(hipMemsetAsync(b, 0, e64.first * sizeof(float), s));      // the all-zero input cube
  const auto& Ls = net->layers; const LayerW &Lin = Ls[kLayerIn], &Ld1 = Ls[kLayerResample1];
  // a stage's three blocks from its input's response on; x_nonneg as in the forward pass (bit-identical either way)
  auto blocks = [&](const StageOffsets& e, int l0, auto launch) {
    const float* x = b + e.first;
    for (int i = 0, rc; i < 3; ++i, x = b + e.o[i - 1]) {
      const BlockW w = block_weights(Ls, l0 + 5 * i);
      for (int which = 0; which < 2; ++which)
        if ((rc = launch(x, b + e.t[i], b + e.o[i], w.p, 1, which, s, true, nullptr))) return rc;
    }
    return 0;
  };
  int rc = launch_conv_in_row(b, b + e64.first, Lin.w_tf, Lin.bias, 1, Lin.def.relu, s);
  if (!rc) rc = blocks(e64, kLayerVrn1, launch_vrn16_row);
  if (rc) return rc;
  net->E64 = b;
  // 32^3: down_1 and the three C = 32 blocks (the kernels' sums do not depend on the tile variant a launch size picks)
  if (Ld1.w_row) {
    rc = launch_down1_row(b + e64.o[2], b + e32.first, Ld1.w_row, Ld1.bias, 1, Ld1.def.relu, s);
    if (!rc) rc = blocks(e32, kLayerVrn2, [](auto... a) { return launch_vrn32_row(a...); });
    if (rc) return rc;
    net->E32 = b;
  }
  return 0;
}

// A layer's buffers in the weight blob as byte offsets (kNone: it has none): TF weights, bias, packed MFMA weights and at most one
// LDS image — of the row kernel that takes the layer (up_2 / down_1; up_1; down_2) or, kept with conv1_1, of a C = 64 / C = 32 block
enum Image { IMG_NONE, IMG_ROW, IMG_UP1, IMG_DOWN2, IMG_VRN64, IMG_VRN32 };
struct LayerBufs { size_t w, bias, mfma, image, block_floats; Image kind; };
constexpr size_t kNone = ~(size_t)0;
static LayerBufs layer_buffers(const LayerDef& d, Arena& a) {
  const int m = mode_of(d);
  const bool block = strcmp(d.name, "conv1_1") == 0;
  LayerBufs b;
  b.kind = row_image_floats(d.cin, d.cout, d.k, m) > 0 ? IMG_ROW
           : d.tconv && d.k == 3 && d.cin == 64 && d.cout == 32 ? IMG_UP1
           : !d.tconv && d.stride == 2 && d.k == 3 && d.cin == 32 && d.cout == 64 ? IMG_DOWN2
           : block && d.cin == 64 && d.cout == 16 ? IMG_VRN64
           : block && d.cin == 32 && d.cout == 8 ? IMG_VRN32 : IMG_NONE;
  const size_t image[] = {0, row_image_floats(d.cin, d.cout, d.k, m), up1_image_floats(), down2_image_floats(), vrn64_image_floats(), vrn32_image_floats()};
  auto take = [&a](size_t floats) { return floats ? a.take(floats * sizeof(float), 256) : kNone; };   // 256-byte aligned sub-buffers
  b.w = take((size_t)d.k * d.k * d.k * d.cin * d.cout);
  b.bias = take(d.bias ? d.cout : 0);
  b.mfma = take(mfma_packed_floats(d.cin, d.cout, d.k, m));
  b.block_floats = b.kind >= IMG_VRN64 ? image[b.kind] : 0;   // a block's image goes behind all layers (place_weights)
  b.image = take(b.block_floats ? 0 : image[b.kind]);
  return b;
}

// the weight blob: every layer's buffers counted, allocated and filled from the caller's tensors
static int place_weights(pcgc_net* net, const std::vector<LayerDef>& table, const float* const* params, hipStream_t s) {
  Arena arena;
  std::vector<LayerBufs> bufs;
  for (const auto& d : table) bufs.push_back(layer_buffers(d, arena));
  for (auto& b : bufs) if (b.block_floats) b.image = arena.take(b.block_floats * sizeof(float), 256);
  PCGC_CHECK_HIP(hipMalloc(&net->blob, arena.take(0, 256)));
  auto at = [net](size_t off) { return off == kNone ? nullptr : reinterpret_cast<float*>(reinterpret_cast<char*>(net->blob) + off); };
  int pi = 0, rc = 0;
  for (size_t l = 0; l < table.size(); ++l) {
    const LayerDef& d = table[l]; const LayerBufs& b = bufs[l];
    hipError_t e = hipMemcpyAsync(at(b.w), params[pi++], (size_t)d.k * d.k * d.k * d.cin * d.cout * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { set_error("weight copy failed: %s", hipGetErrorString(e)); return -100; }
    if (d.bias) e = hipMemcpyAsync(at(b.bias), params[pi++], d.cout * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) { set_error("bias copy failed: %s", hipGetErrorString(e)); return -100; }
    if (b.mfma != kNone) rc = pack_weights_mfma(at(b.w), at(b.mfma), d.cin, d.cout, d.k, mode_of(d), s);
    if (!rc && b.kind == IMG_ROW) rc = launch_row_image(at(b.w), at(b.image), mode_of(d), s);
    if (!rc && b.kind == IMG_UP1) rc = launch_up1_image(at(b.w), at(b.image), s);
    if (!rc && b.kind == IMG_DOWN2) rc = launch_down2_image(at(b.w), at(b.image), s);
    if (rc) return rc;
    net->layers.push_back(LayerW{d, at(b.w), at(b.bias), at(b.mfma), at(b.image)});
  }
  for (size_t l = 0; l < table.size() && !rc; ++l) {          // the blocks' images: every layer of the block is in place
    if (!bufs[l].block_floats) continue;
    const BlockW w = block_weights(net->layers, l);
    rc = bufs[l].kind == IMG_VRN64 ? launch_vrn64_image(w.p, at(bufs[l].image), s) : launch_vrn32_image(w.p, at(bufs[l].image), s);
  }
  return rc;
}

extern "C" {

int pcgc_version(void) { return 1; }
const char* pcgc_last_error(void) { return pcgc::g_err; }

int pcgc_net_param_count(int kind) {
  int n = 0;
  for (const auto& d : layer_table(kind)) n += 1 + d.bias;
  return n;
}

int pcgc_net_create(int kind, const float* const* params, int n_params, pcgc_stream_t stream, pcgc_net** out) {
  hipStream_t s = (hipStream_t)stream;
  auto table = layer_table(kind);
  PCGC_REQUIRE(!table.empty(), "pcgc_net_create: unknown kind %d", kind);
  PCGC_REQUIRE(n_params == pcgc_net_param_count(kind), "pcgc_net_create: kind %d expects %d tensors, got %d", kind,
               pcgc_net_param_count(kind), n_params);
  PCGC_REQUIRE(out != nullptr, "pcgc_net_create: out is NULL");
  PCGC_REQUIRE((kind != PCGC_NET_ANALYSIS && kind != PCGC_NET_SYNTHESIS) || layer_indices_match(table),
               "pcgc_net_create: the layer table of kind %d does not match the kLayer* indices", kind);
  pcgc_net* net = new pcgc_net();
  net->kind = kind; net->algo = 0;
  net->chunk = getenv("PCGC_CHUNK_CUBES") ? atoi(getenv("PCGC_CHUNK_CUBES")) : 0;
  int rc = place_weights(net, table, params, s);
  if (!rc && kind == PCGC_NET_ANALYSIS) rc = make_empty_responses(net, s);
  if (rc) { pcgc_net_destroy(net); return rc; }
  *out = net;
  return 0;
}

void pcgc_net_destroy(pcgc_net* net) {
  if (!net) return;
  if (net->blob) (void)hipFree(net->blob);
  if (net->empty_blob) (void)hipFree(net->empty_blob);
  delete net;
}

int pcgc_net_set_profiling(pcgc_net* net, int on) {
  PCGC_REQUIRE(net, "pcgc_net_set_profiling: net is NULL");
  net->profiling = on != 0;
  return 0;
}

// One line per launch since the last report: "layer kernel cin cout k mode B Din ms\n".  Synchronises the stream's
// recorded events (profiling aid, not part of the data path).
int pcgc_net_profile_report(pcgc_net* net, char* buf, size_t cap, size_t* needed) {
  PCGC_REQUIRE(net && needed, "pcgc_net_profile_report: NULL argument");
  std::string out;
  for (auto& r : net->prof) {
    float ms = 0.f;
    (void)hipEventSynchronize(r.t1);
    (void)hipEventElapsedTime(&ms, r.t0, r.t1);
    const auto& d = net->layers[r.layer].def;
    char line[256];
    snprintf(line, sizeof(line), "%d %s %s %d %d %d %d %d %d %.6f\n", r.layer, d.name, kKernName[r.kern], d.cin, d.cout, d.k, mode_of(d), r.B,
             r.Din, ms);
    out += line;
    (void)hipEventDestroy(r.t0);
    (void)hipEventDestroy(r.t1);
  }
  net->prof.clear();
  *needed = out.size() + 1;
  if (buf && cap >= out.size() + 1) memcpy(buf, out.c_str(), out.size() + 1);
  return 0;
}

// Test aid for the exact skipping of empty space (analysis, 64^3 stage): a device word the kernels add 1 to for every
// wave tile they copy from the empty-cube response instead of computing it (NULL: off).
int pcgc_net_set_skip_counter(pcgc_net* net, unsigned* device_counter) {
  PCGC_REQUIRE(net, "pcgc_net_set_skip_counter: net is NULL");
  net->skip_counter = device_counter;
  return 0;
}

int pcgc_rowocc(const float* x, unsigned long long* rowocc, int B, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(x && rowocc && B > 0, "pcgc_rowocc: bad arguments");
  return launch_rowocc(x, rowocc, B, (hipStream_t)stream);
}

int pcgc_net_set_algo(pcgc_net* net, int algo) {
  PCGC_REQUIRE(net && (algo == 0 || algo == 1), "pcgc_net_set_algo: bad arguments");
  net->algo = algo;
  return 0;
}

size_t pcgc_net_workspace_bytes(const pcgc_net* net, int B, int D) {
  if (!net || B <= 0) return 0;
  return make_plan(net, B, D).total + 256;                 // + the room to align the caller's pointer
}

int pcgc_net_forward(const pcgc_net* net, const float* x, float* out0, float* out1, int B, int D,
                     float scale_lower_bound, void* workspace, size_t workspace_bytes, pcgc_stream_t stream) {
  PCGC_REQUIRE(net != nullptr, "pcgc_net_forward: net is NULL");
  if (B == 0) return 0;                                    // empty batch: valid no-op
  PCGC_REQUIRE(B > 0 && D > 0, "pcgc_net_forward: bad B=%d D=%d", B, D);
  const int div = net->kind == PCGC_NET_ANALYSIS ? 4 : (net->kind == PCGC_NET_HYPER_ENCODER ? 2 : 1);
  PCGC_REQUIRE(D % div == 0, "pcgc_net_forward: input size %d must be a multiple of %d for this transform", D, div);
  PCGC_REQUIRE(x && out0 && (net->kind != PCGC_NET_HYPER_DECODER || out1), "pcgc_net_forward: NULL tensor");
  const NetPlan p = make_plan(net, B, D);
  PCGC_REQUIRE(workspace_bytes >= p.total + 256, "pcgc_net_forward: workspace too small (%zu < %zu)", workspace_bytes, p.total + 256);
  char* ws = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  if (net->kind == PCGC_NET_ANALYSIS || net->kind == PCGC_NET_SYNTHESIS)
    return forward_autoencoder(net, p, x, out0, B, D, ws, workspace_bytes - (size_t)(ws - static_cast<char*>(workspace)), (hipStream_t)stream);
  for (int b0 = 0; b0 < B; b0 += kHyperChunk) {
    const int nb = std::min(B - b0, kHyperChunk);
    int rc = forward_chunk(net, x + (size_t)b0 * in_floats_per_cube(net->kind, D),
                           out0 + (size_t)b0 * out_floats_per_cube(net->kind, D, 0),
                           out1 ? out1 + (size_t)b0 * out_floats_per_cube(net->kind, D, 1) : nullptr, nb, D, scale_lower_bound,
                           region<float>(ws, p, R_F1), region<float>(ws, p, R_F2), region<float>(ws, p, R_F3), (hipStream_t)stream);
    if (rc) return rc;
  }
  return 0;
}

// One _VoxceptionResNet block (model_voxception.py:56-68) on NDHWC tensors.  C = 16 at D = 64 runs the row kernels
// of vrn_row.hip (layout conversion in, two kernels, conversion out); other shapes run the generic layer kernels.
size_t pcgc_vrn_workspace_bytes(int B, int D, int C) {
  if (B <= 0 || D <= 0 || C <= 0) return 0;
  const size_t vox = (size_t)B * D * D * D;
  return vox * (size_t)(C + C) * sizeof(float) + 256;      // row path: x in Q4 + t12; generic path: 3 x C/4 scratch
}

int pcgc_vrn_fwd_train_supported(int D, int C) { return (D == 64 && C == 16) || (D == 32 && C == 32); }

int pcgc_vrn_fwd_train(const float* x, const float* const* params, float* t11, float* t21, float* t22, float* pre, float* out, int B,
                       int D, int C, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(x && params && t11 && t21 && t22 && pre && out, "pcgc_vrn_fwd_train: NULL tensor");
  PCGC_REQUIRE(pcgc_vrn_fwd_train_supported(D, C), "pcgc_vrn_fwd_train: no fused kernel for D=%d C=%d (run the block layer by layer)", D, C);
  PCGC_REQUIRE(out != x, "pcgc_vrn_fwd_train: the reverse pass needs x, out must not alias it");
  if (D == 32) return launch_vrn32_row_train(x, t11, t21, t22, pre, out, params, B, (hipStream_t)stream);
  return launch_vrn16_row_train(x, t11, t21, t22, pre, out, params, B, (hipStream_t)stream);
}

int pcgc_vrn_fwd_train_signs_supported(int D, int C) { return (D == 64 && C == 16) || (D == 32 && C == 32); }

int pcgc_vrn_fwd_train_signs(const float* x, const float* const* params, float* t11, float* t21, float* t22, int32_t* pre_signs,
                             float* out, int B, int D, int C, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(x && params && t11 && t21 && t22 && pre_signs && out, "pcgc_vrn_fwd_train_signs: NULL tensor");
  PCGC_REQUIRE(pcgc_vrn_fwd_train_signs_supported(D, C), "pcgc_vrn_fwd_train_signs: D=%d C=%d (D = 64 with C = 16, D = 32 with C = 32)", D, C);
  PCGC_REQUIRE(out != x, "pcgc_vrn_fwd_train_signs: the reverse pass needs x, out must not alias it");
  if (D == 32) return launch_vrn32_row_train(x, t11, t21, t22, nullptr, out, params, B, (hipStream_t)stream, pre_signs);
  return launch_vrn16_row_train(x, t11, t21, t22, nullptr, out, params, B, (hipStream_t)stream, pre_signs);
}

// the same with x / out in the Q4 layout [b][d][h][C/4][w][4] (the training step's 64^3 stage, Trainer(q4=True))
int pcgc_vrn_fwd_train_q4(const float* x, const float* const* params, float* t11, float* t21, float* t22, int32_t* pre_signs,
                          float* out, int B, int D, int C, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(x && params && t11 && t21 && t22 && pre_signs && out, "pcgc_vrn_fwd_train_q4: NULL tensor");
  PCGC_REQUIRE(D == 64 && C == 16, "pcgc_vrn_fwd_train_q4: D=%d C=%d (D = 64 with C = 16 only)", D, C);
  PCGC_REQUIRE(out != x, "pcgc_vrn_fwd_train_q4: the reverse pass needs x, out must not alias it");
  return launch_vrn16_row_train(x, t11, t21, t22, nullptr, out, params, B, (hipStream_t)stream, pre_signs, true);
}

// NDHWC [B][D^3][C] <-> Q4 [B][D][D][C/4][D][4] (to_q4 = 1 / 0); C a multiple of 4
int pcgc_layout_q4(const float* src, float* dst, int B, int D, int C, int to_q4, pcgc_stream_t stream) {
  if (B == 0) return 0;
  PCGC_REQUIRE(src && dst && src != dst && B > 0 && D > 0 && C >= 4 && C % 4 == 0, "pcgc_layout_q4: bad arguments");
  return launch_q4_convert(src, dst, B, D, C, to_q4, (hipStream_t)stream);
}

int pcgc_vrn_fwd(const float* x, const float* const* params, float* out, int B, int D, int C, void* workspace,
                 size_t workspace_bytes, pcgc_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return 0;
  PCGC_REQUIRE(x && params && out, "pcgc_vrn_fwd: NULL tensor");
  PCGC_REQUIRE(B > 0 && D > 0 && C >= 4 && C % 4 == 0, "pcgc_vrn_fwd: bad B=%d D=%d C=%d", B, D, C);
  PCGC_REQUIRE(workspace && workspace_bytes >= pcgc_vrn_workspace_bytes(B, D, C), "pcgc_vrn_fwd: workspace too small");
  float* ws = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const size_t vox = (size_t)B * D * D * D;
  if ((C == 16 && D == 64) || (C == 32 && D == 32) || (C == 64 && D == 16)) {
    float* xq = ws;
    float* t12 = ws + vox * C;
    int rc;
    if ((rc = launch_q4_convert(x, xq, B, D, C, 1, s))) return rc;
    for (int which = 0; which < (C == 64 ? 3 : 2); ++which)
      if ((rc = C == 16 ? launch_vrn16_row(xq, t12, xq, params, B, which, s)
                        : (C == 32 ? launch_vrn32_row(xq, t12, xq, params, B, which, s) : launch_vrn64_row(xq, t12, xq, params, B, which, s))))
        return rc;
    return launch_q4_convert(xq, out, B, D, C, 0, s);
  }
  pcgc_net net;
  net.kind = -1; net.algo = 1; net.chunk = 0; net.blob = nullptr;
  std::vector<LayerDef> defs;
  push_vrn(defs, C);
  for (int i = 0; i < 5; ++i) net.layers.push_back(LayerW{defs[i], params[2 * i], params[2 * i + 1], nullptr});
  Exec E{&net, s, B};
  const size_t q = vox * (C / 4);
  return E.vrn(0, x, out, D, C, ws, ws + q, ws + 2 * q);
}

#ifdef PCGC_EXPERIMENTS
// experiments (tools/exp/t_ablate.py; builds with PCGC_EXPERIMENTS=1 only — the default libpcgc_hip.so neither exports these
// nor has the global they set): one launch of the 64^3 row kernel A (which = 0) or BC (1) on Q4 tensors already on the device
int pcgc_exp_vrn16_row(const float* xq, float* t12, float* outq, const float* const* params, int B, int which, int x_nonneg, int abl,
                       void* stream) {
  pcgc::g_vrn16_abl = abl;
  const int rc = launch_vrn16_row(xq, t12, outq, params, B, which, (hipStream_t)stream, x_nonneg != 0);
  pcgc::g_vrn16_abl = 0;
  return rc;
}

// the ablation switches for every later launch of the 64^3 row kernels (training variants included)
int pcgc_exp_set_vrn16_ablation(int abl) { pcgc::g_vrn16_abl = abl; return 0; }
#endif

int pcgc_conv3d_fwd(const float* x, const float* kernel, const float* bias, float* y, int B, int D, int Cin, int Cout,
                    int ksize, int stride, int transposed, int relu, int algo, pcgc_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return 0;
  PCGC_REQUIRE(x && kernel && y, "pcgc_conv3d_fwd: NULL tensor");
  PCGC_REQUIRE(ksize >= 1 && ksize <= 9 && (ksize & 1) && (stride == 1 || stride == 2) && B >= 0 && D > 0 && Cin > 0 && Cout > 0,
               "pcgc_conv3d_fwd: unsupported geometry k=%d stride=%d", ksize, stride);
  PCGC_REQUIRE(!transposed || stride == 2, "pcgc_conv3d_fwd: transposed conv needs stride=2");
  PCGC_REQUIRE(stride == 1 || transposed || D % 2 == 0, "pcgc_conv3d_fwd: stride-2 conv needs even D");
  if (B == 0) return 0;
  ConvArgs a;
  a.x = x; a.w = kernel; a.bias = bias; a.y = y; a.res = nullptr;
  a.B = B; a.Din = D; a.Dout = transposed ? 2 * D : D / stride;
  a.Cin = Cin; a.Cout = Cout; a.x_cs = Cin; a.x_co = 0; a.y_cs = Cout; a.y_co = 0;
  a.ksize = ksize; a.mode = transposed ? 2 : (stride == 2 ? 1 : 0); a.relu = relu; a.absval = 0; a.lower_bound = 0.f;
  a.w2 = nullptr; a.bias2 = nullptr; a.y2 = nullptr; a.y2_cs = 0; a.cout2 = 0;
  if (algo == 3) {
    int rc = launch_conv_valu(a, s, true);
    PCGC_REQUIRE(rc != 0, "pcgc_conv3d_fwd: no VALU tile kernel for this shape");
    return rc < 0 ? rc : 0;
  }
  if (algo == 0 && (Cin == 1 || Cout == 1)) {            // conv_in / deconv_out: the LDS-tiled VALU kernel, as pcgc_net_forward picks
    const int rc = launch_conv_valu(a, s, true);
    if (rc != 0) return rc < 0 ? rc : 0;
  }
  if (algo != 1 && launch_conv_mfma(a, nullptr, s, false) == 1) {
    float* packed = nullptr;
    const size_t n = mfma_packed_floats(Cin, Cout, ksize, a.mode);
    PCGC_CHECK_HIP(hipMallocAsync((void**)&packed, n * sizeof(float), s));
    int rc = pack_weights_mfma(kernel, packed, Cin, Cout, ksize, a.mode, s);
    if (!rc) { rc = launch_conv_mfma(a, packed, s, true); rc = rc < 0 ? rc : 0; }
    (void)hipFreeAsync(packed, s);
    return rc;
  }
  PCGC_REQUIRE(algo != 2, "pcgc_conv3d_fwd: no MFMA kernel for Cin=%d Cout=%d k=%d stride=%d transposed=%d D=%d", Cin,
               Cout, ksize, stride, transposed, D);
  return launch_conv_direct(a, s);
}

}  // extern "C"
