// Model handles and forward orchestration (host code) + the extern "C" ABI of include/sapcu.h.
//
// A forward is a fixed sequence of launches on the caller's stream over caller-owned workspace, one chunk of patches at a time (the
// chunk size bounds the footprint: fn_plan / fd_plan).  Each forward has ONE description of its workspace, fn_ws_layout /
// fd_ws_layout: sapcu_workspace_bytes is that function on a null base, the forward carves the caller's buffer with it.
//  * In split-f16 mode (the default; SAPCU_GEMM=f32 or a weight outside the f16 range falls back to the exact-f32 MFMA GEMM) the 1x1
//    convolutions / Linears run as 3 x f16 MFMA GEMMs on weights split once at model build, neuron loops fused as epilogues; tensors
//    that only feed another GEMM travel as split rows.  Every GEMM, a handle's or a raw entry point's, is a descriptor filled by the
//    Gemm builder and sent through gemm_route, the one place that says which of the five GEMM kernels a descriptor reaches.
//  * fn: per block fc1 and q|k|v GEMMs over all rows of the chunk, then the edge chain — ONE kernel with the activations in LDS
//    (fn_edge_chain.hip) for the shapes it takes, else five kernels over [rows * k, d] tensors in HBM — and out_proj . fc2 folded
//    into one GEMM at model build.
//  * fd: the encoder as ONE LDS-resident kernel per patch (fd_encoder.hip) up to 48 points; larger patches run the per-stage
//    front through HBM and multi_scale_conv either from x0 (fd_msc_kernel) or as a GEMM over T spike slabs.
// The irregular parts (in-patch kNN, gathers, softmax over neighbours, pooling) are the small kernels of patch_ops.hip.
#include <stdarg.h>
#include <stdlib.h>

#include <memory>
#include <new>
#include <vector>

#include "common.h"
#include "ops.h"

namespace sapcu {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---------------------------------------------------------------- slot tables (== packing.py)
enum FnSlot {
    FN_STEM_W = 0, FN_STEM_B, FN_STEM_LIF,
    FN_BLK0 = 3,   // 21 slots per block, 3 blocks
    FN_FINAL_W = FN_BLK0 + 63, FN_FINAL_B, FN_FINAL_LIF,
    FN_FCOUT_W, FN_FCOUT_B,
    FN_MLP0_W, FN_MLP0_B, FN_MLP1_W, FN_MLP1_B, FN_MLP2_W, FN_MLP2_B,
    FN_HEAD_W, FN_HEAD_B, FN_LN_W, FN_LN_B,
    FN_SLOTS
};
enum FnBlkSlot {
    B_FC1_W = 0, B_FC1_B, B_SNN1,
    B_QKV_W, B_QKV_B, B_QKV_LIF,
    B_DELTA_W, B_DELTA_B, B_DELTA_LIF,
    B_DELTA2_W, B_DELTA2_B, B_DELTA2_LIF,
    B_GAMMA_W, B_GAMMA_B, B_GAMMA_LIF,
    B_GAMMA2_W, B_GAMMA2_B,
    B_OUT_W, B_OUT_B,
    B_FC2_W, B_FC2_B,
    B_SLOTS
};
static_assert(B_SLOTS == 21, "fn block slot count");
static_assert(FN_SLOTS == 81, "fn slot count");

enum FdSlot {
    FD_E0_W = 0, FD_E0_B,
    FD_FUSE_W, FD_FUSE_B, FD_SNN0,
    FD_EDGE1_W, FD_EDGE1_SHIFT, FD_SNN1,
    FD_EDGE2_W, FD_EDGE2_SHIFT, FD_SNN2,
    FD_EDGE3_W, FD_EDGE3_SHIFT, FD_SNN3,
    FD_MSC_W, FD_MSC_B,
    FD_TI_W, FD_SNNFC,
    FD_FCIN_W, FD_FCIN_B,
    FD_R0_FC0_W, FD_R0_FC0_B, FD_R0_FC4_W, FD_R0_FC4_B, FD_R0_PROJ_W, FD_R0_PROJ_B,
    FD_R1_FC0_W, FD_R1_FC0_B, FD_R1_FC4_W, FD_R1_FC4_B, FD_R1_PROJ_W, FD_R1_PROJ_B,
    FD_QKV_W, FD_QKV_B,
    FD_WO_T, FD_BO, FD_LN_W, FD_LN_B, FD_WH_T, FD_BH, FD_WD, FD_BD,
    FD_SLOTS
};
static_assert(FD_SLOTS == 42, "fd slot count");

}  // namespace sapcu

struct sapcu_model {
    int kind = 0;
    // fn
    int kv[3] = {0, 0, 0};
    // fd
    int k = 0, nscale = 0;
    int ks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t* ks_dev = nullptr;
    int* gate_dev = nullptr;
    // split-f16 GEMM path: the whole blob pre-split (same indexing), activation-range overflow counter
    bool sf16 = true;
    void* w16_hi = nullptr;
    void* w16_lo = nullptr;
    void* chain_w = nullptr;   // fn: fc_delta2 | fc_gamma | fc_gamma2 of the three blocks in MFMA-fragment order (fn_edge_chain.hip, chain_w_off)
    int* ovf_dev = nullptr;
    // common
    int emb = 0, T = 0, heads = 0;
    int64_t chunk = 0;         // patches per chunk: SAPCU_CHUNK, or 0 = from the workspace budget (ws_budget bytes per forward)
    int64_t ws_budget = 0;
    // parity / ablation switches, read from the environment ONCE, at sapcu_model_create (read_env_switches; a handle is immutable
    // afterwards: a forward never calls getenv; tests build a second handle under another environment instead of flipping it mid-process)
    bool opt_bt = true;               // SAPCU_BT=0: split-row GEMMs on the ring kernel only
    bool opt_chain = true;            // SAPCU_CHAIN=0: fn blocks as the five-kernel edge chain
    bool opt_chain_wide = false;      // SAPCU_CHAIN=wide: the fused chain with 64-bit gather addresses (the form tensors >= 4 GiB take)
    bool opt_chain_fill = true;       // SAPCU_CHAIN_FILL=0: the d = 512 fused chain in plain groups of five points, four slots of 64 idle
    bool opt_chain_trim = true;       // SAPCU_CHAIN_TRIM=0: the fused chain's fc_delta on the VALU and its spare-slot points summed in every lane group
    bool opt_shortk = true;           // SAPCU_SHORTK=0: fc1 / conv_final on gemm_sf16_kernel instead of gemm_shortk.hip
    bool opt_fn_maxfuse = true;       // SAPCU_FN_MAXFUSE=0: conv_final GEMM + rowgroup_max
    bool opt_fn_fold_out = true;      // SAPCU_FN_FOLD_OUT=0: fn blocks end with out_proj and fc2 as two GEMMs instead of the folded one
    bool opt_fd_maxfuse = true;       // SAPCU_FD_MAXFUSE=0: multi_scale_conv GEMM + rowgroup_max
    bool opt_fd_split = true;         // SAPCU_FD_SPLIT=0: fd spikes as f32 rows for every step
    bool opt_fd_fused = true;         // SAPCU_FD_FUSED=0: fd encoder on the per-stage kernels (through HBM) instead of fd_encoder.hip
    bool opt_fd_x0 = true;            // SAPCU_FD_X0=0: the per-stage path writes T spike slabs for the big-tile GEMM instead of x0 for fd_msc_kernel
    // fd, fused encoder (fd_encoder.hip): scale_fusion | EdgeConv 1-3 | multi_scale_conv in MFMA-fragment order, clamped neuron
    // parameters of the 960 encoder channels
    void* fde_w = nullptr;
    int64_t fde_off[5] = {0, 0, 0, 0, 0};     // offsets (halves) of the five matrices inside fde_w
    float* fde_nprm = nullptr;
    float* blob = nullptr;
    int64_t blob_floats = 0;   // the caller's blob + (fn) the folded out_proj . fc2 parameters appended at model build
    // fn: fc2(out_proj(x)) of block l as ONE affine map, W' = W_fc2 . W_out [64, d] and b' = W_fc2 . b_out + b_fc2 [64]: offsets (floats)
    // into blob, behind the caller's slots, so that the split-f16 planes and the weight range guard cover them like every other slot
    int64_t fold_w[3] = {0, 0, 0}, fold_b[3] = {0, 0, 0};
    std::vector<int64_t> dir;
    const float* p(int slot) const { return blob + dir[slot]; }
};

namespace sapcu {

static inline int64_t imax(int64_t a, int64_t b) { return a > b ? a : b; }
static inline int imin(int a, int b) { return a < b ? a : b; }

#define SAPCU_TRY(expr)                 \
    do {                                \
        int _rc = (expr);               \
        if (_rc != SAPCU_OK) return _rc; \
    } while (0)

// ---------------------------------------------------------------- the GEMM router
// Which launcher a filled descriptor reaches: the ONLY statement of the order (the _ok / _accepts predicates stay with their kernels).
//   have16        split weights are attached (g.w16_hi / w16_lo).  Handle: split-f16 mode and g.w inside the handle's blob; raw entry
//                 points: the caller gave a w16_ws scratch.
//   allow_bt      handle: not created under SAPCU_BT=0; raw: a_split_rows / split_rows != 2.
//   allow_shortk  handle: not created under SAPCU_SHORTK=0; raw sapcu_gemm_f32: SAPCU_SHORTK read at the call.  The posenc GEMM cannot get
//                 there whatever it passes: gemm_shortk_ok refuses EPI_LIF_ATTN.
// The first row that applies decides:
//   have16  a_split  allow_bt && gemm_sf16_bt_ok                    big tile
//   have16  a_split  gemm_sf16_ring_accepts                         ring (every r == 0 call ends here: SAPCU_OK without a launch)
//   have16  a_split                                                 refused, the ring's text
//   have16           allow_shortk && gemm_shortk_ok                 short K
//   have16           max_out                                        refused: "a direct max output needs the short-K kernel"
//   have16           k % 64 == 0                                    f32 A, split per tile (its K step is 64)
//   have16           c_split | c2_split                             refused: "split-row output needs k % 64 == 0 on the f32-A path"
//           a_split | c_split | c2_split                            refused: "split-row operands need the split-f16 kernels"
//                                                                   exact f32
typedef int (*GemmLauncher)(const GemmArgs&, hipStream_t);

// the launcher, or null with the refusal's text in *why; launches and writes nothing, sets no error
static GemmLauncher gemm_route(const GemmArgs& g, bool have16, bool allow_bt, bool allow_shortk, const char** why) {
    if (have16 && g.a_split) {
        if (allow_bt && gemm_sf16_bt_ok(g)) return launch_gemm_sf16_bt;
        return gemm_sf16_ring_accepts(g, why) ? launch_gemm_sf16_ring : nullptr;
    }
    *why = nullptr;
    if (have16) {
        if (allow_shortk && gemm_shortk_ok(g)) return launch_gemm_shortk;
        if (g.max_out) *why = "run_gemm: a direct max output needs the short-K kernel";
        else if (g.k % 64 == 0) return launch_gemm_sf16;
        else if (g.c_split || g.c2_split) *why = "gemm: split-row output needs k % 64 == 0 on the f32-A path";
    } else if (g.a_split || g.c_split || g.c2_split) {
        *why = "run_gemm: split-row operands need the split-f16 kernels";
    }
    return *why ? nullptr : launch_gemm;
}

// A raw entry point's split scratch for cnt weights: hi (2 cnt B) | lo (2 cnt B) | overflow counter
struct SplitWs {
    _Float16 *hi, *lo;
    int* ovf;
    int64_t cnt;
    SplitWs(void* ws, int64_t cnt_) : hi((_Float16*)ws), lo(hi + cnt_), ovf((int*)(lo + cnt_)), cnt(cnt_) {}
    void attach(GemmArgs& g) const { g.w16_hi = hi; g.w16_lo = lo; g.ovf = ovf; }      // pointers only: nothing is written
    int fill(const float* w, hipStream_t st) const {                                    // zero the counter, split w into the planes
        SAPCU_CHECK_HIP(hipMemsetAsync(ovf, 0, sizeof(int), st));
        return launch_split_weights(w, cnt, hi, lo, ovf, st);
    }
};

// Route and launch; a refusal becomes the thread's error text before anything is launched or written.  raw: the scratch attached to g,
// filled between the two steps — the exact-f32 route leaves it untouched.
static int gemm_run(const GemmArgs& g, bool have16, bool allow_bt, bool allow_shortk, hipStream_t st, const SplitWs* raw = nullptr) {
    const char* why = nullptr;
    const GemmLauncher run = gemm_route(g, have16, allow_bt, allow_shortk, &why);
    SAPCU_CHECK_ARG(run, "%s", why);
    if (raw && run != launch_gemm) SAPCU_TRY(raw->fill(g.w, st));
    return run(g, st);
}

int launch_gemm_split_rows(const GemmArgs& g, hipStream_t st, bool allow_bt) { return gemm_run(g, true, allow_bt, false, st); }

// A descriptor under construction: the ten fields every GEMM has, then one named setter per group an epilogue or a format adds.  The
// rest stays zero; GemmArgs itself (what the kernels take by value) is untouched.
struct Gemm : GemmArgs {
    Gemm(const float* a_, int64_t r_, int k_, int lda_, const float* w_, int n_, const float* bias_, float* c_, int ldc_, int epi_)
        : GemmArgs{} {
        a = a_; r = r_; k = k_; lda = lda_; w = w_; n = n_; bias = bias_; c = c_; ldc = ldc_; epi = epi_;
    }
    Gemm& neuron(const float* params, int steps) { lif = params; lif_T = steps; return *this; }
    Gemm& residual(const float* x, int ld) { resid = x; ldr = ld; return *this; }
    Gemm& split_in(int on = 1) { a_split = on; return *this; }
    Gemm& split_out(int on = 1) { c_split = on; return *this; }
    Gemm& split_out2(int on = 1) { c2_split = on; return *this; }
    // EPI_LIF_ATTN: c2 = q[tab.x] - kf[tab.y] + c, q | kf the first two d-column groups of qkv rows [*, 3 d]
    Gemm& attn(float* c2_, const float* qkv, int d, const int2* tab_) { c2 = c2_; q = qkv; kf = qkv + d; ldq = 3 * d; tab = tab_; return *this; }
    // EPI_*_MAX: keys of the max over groups of m rows; out: the float maxima written directly (short-K kernel, whole patches per row group)
    Gemm& max_rows(unsigned* keys, int m, float* out = nullptr) { max_keys = keys; max_m = m; max_out = out; return *this; }
};

// out_proj followed by fc2 (two affine maps with nothing between them, fn/snn_coder.py:393-394) as one: w_fold [n, d] = w2 . w1 and
// b_fold [n] = w2 . b1 + b2 for w1 [d, d], b1 [d] (out_proj) and w2 [n, d], b2 [n] (fc2), BatchNorm already folded.  HOST pointers;
// every sum in f64 over ascending j, rounded to f32 once.  Runs once per model (n d d products).
static void fold_affine_f64(const float* w1, const float* b1, const float* w2, const float* b2, int d, int n, float* w_fold,
                            float* b_fold) {
    std::vector<double> acc((size_t)d);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < d; ++k) acc[k] = 0.0;
        double bs = 0.0;
        for (int j = 0; j < d; ++j) {
            const double a = (double)w2[(int64_t)i * d + j];
            const float* row = w1 + (int64_t)j * d;
            for (int k = 0; k < d; ++k) acc[k] += a * (double)row[k];
            bs += a * (double)b1[j];
        }
        for (int k = 0; k < d; ++k) w_fold[(int64_t)i * d + k] = (float)acc[k];
        b_fold[i] = (float)(bs + (double)b2[i]);
    }
}

static bool env_is(const char* name, const char* value) {
    const char* e = getenv(name);
    return e && strcmp(e, value) == 0;
}

// the SAPCU_* switches of a handle (include/sapcu.h), read at sapcu_model_create and nowhere else
static void read_env_switches(sapcu_model* m) {
    m->sf16 = !env_is("SAPCU_GEMM", "f32");
    m->opt_bt = !env_is("SAPCU_BT", "0");
    m->opt_chain = !env_is("SAPCU_CHAIN", "0");
    m->opt_chain_wide = env_is("SAPCU_CHAIN", "wide");
    m->opt_chain_fill = !env_is("SAPCU_CHAIN_FILL", "0");
    m->opt_chain_trim = !env_is("SAPCU_CHAIN_TRIM", "0");
    m->opt_shortk = !env_is("SAPCU_SHORTK", "0");
    m->opt_fn_maxfuse = !env_is("SAPCU_FN_MAXFUSE", "0");
    m->opt_fn_fold_out = !env_is("SAPCU_FN_FOLD_OUT", "0");
    m->opt_fd_maxfuse = !env_is("SAPCU_FD_MAXFUSE", "0");
    m->opt_fd_split = !env_is("SAPCU_FD_SPLIT", "0");
    m->opt_fd_fused = !env_is("SAPCU_FD_FUSED", "0");
    m->opt_fd_x0 = !env_is("SAPCU_FD_X0", "0");
    const char* ce = getenv("SAPCU_CHUNK");
    m->chunk = ce ? atoll(ce) : 0;
    if (m->chunk < 0) m->chunk = 0;
    // workspace budget per forward (the caller owns the buffer; sapcu_workspace_bytes reports what a batch needs under it):
    // 20 GiB holds the whole 4096-patch benchmark batch at M = 48 in one chunk (16.9 GB fn, 6.7 GB fd) and cuts the reference's
    // default M = 100 (8.5 MB per patch) into chunks of ~2400 patches instead of a 35 GB workspace
    const char* be = getenv("SAPCU_WS_BUDGET_MB");
    m->ws_budget = (be ? atoll(be) : 20480) * (int64_t)(1 << 20);
    if (m->ws_budget < (int64_t)(64 << 20)) m->ws_budget = (int64_t)(64 << 20);
}

// a handle and everything it owns on the device (a failed sapcu_model_create and sapcu_model_destroy)
static void free_model(sapcu_model* m) {
    void* const owned[] = {m->w16_hi, m->w16_lo, m->chain_w, m->ovf_dev, m->blob, m->ks_dev, m->gate_dev, m->fde_w, m->fde_nprm};
    for (void* p : owned)
        if (p) (void)hipFree(p);
    delete m;
}

// The handle's split planes and overflow counter attached to a descriptor whose weights are the handle's (split-f16 mode); says
// whether it did.  Anything else runs on exact f32.
static bool attach_split_weights(const sapcu_model* m, GemmArgs& g) {
    if (!m->sf16 || g.w < m->blob || g.w >= m->blob + m->blob_floats) return false;
    const int64_t off = g.w - m->blob;
    g.w16_hi = (const _Float16*)m->w16_hi + off;
    g.w16_lo = (const _Float16*)m->w16_lo + off;
    g.ovf = m->ovf_dev;
    return true;
}

static int run_gemm(const sapcu_model* m, GemmArgs g, hipStream_t st) {
    const bool have16 = attach_split_weights(m, g);
    return gemm_run(g, have16, m->opt_bt, m->opt_shortk, st);
}

static int tap_copy(void* const* taps, int which, int64_t dst_off_bytes, const void* src, int64_t bytes,
                    hipStream_t st) {
    if (!taps || !taps[which] || bytes == 0) return SAPCU_OK;
    SAPCU_CHECK_HIP(hipMemcpyAsync((char*)taps[which] + dst_off_bytes, src, (size_t)bytes, hipMemcpyDeviceToDevice, st));
    return SAPCU_OK;
}

// a [T][cb] tensor of `row` floats per patch into its tap, laid out [T][b]: this chunk's patches [s, s + cb) of every step
static int tap_copy_steps(void* const* taps, int which, int T, int64_t b, int64_t s, int64_t cb, int64_t row, const float* src,
                          hipStream_t st) {
    for (int t = 0; t < T; ++t) SAPCU_TRY(tap_copy(taps, which, ((int64_t)t * b + s) * row * 4, src + (int64_t)t * cb * row, cb * row * 4, st));
    return SAPCU_OK;
}

// the caller's workspace against a layout's bytes + the 256 the align-up of its pointer may cost
static int check_workspace(const char* who, int64_t ws_bytes, size_t layout_bytes) {
    if (ws_bytes >= (int64_t)layout_bytes + 256) return SAPCU_OK;
    set_error("%s: workspace %lld B < required %lld B", who, (long long)ws_bytes, (long long)layout_bytes + 256);
    return SAPCU_ERR_WORKSPACE;
}

// ============================================================================ fn
struct FnPlan {
    int64_t cb;       // patches per chunk
    int kk[3], kmx;   // neighbours per block (k clamped to the patch), the largest of them
    int64_t edge_floats, edge_floats23;   // per-chunk size of edge buffer 1 (also conv_final's output) and of buffers 2, 3
};

// does block l run its edge chain fused (fn_edge_chain.hip)?  The workspace plan and the forward use the same answer
// (SAPCU_CHAIN=0 at model creation keeps the five-kernel chain).
static bool fn_block_fused(const sapcu_model* m, int l, int mp) {
    return m->sf16 && m->chain_w && m->opt_chain && fn_edge_chain_ok(128 << l, imin(m->kv[l], mp));
}

// the largest neighbour count of the three blocks, each clamped to the patch
static int fn_kmax(const sapcu_model* m, int mp) {
    int kmx = 1;
    for (int l = 0; l < 3; ++l) kmx = kmx > imin(m->kv[l], mp) ? kmx : imin(m->kv[l], mp);
    return kmx;
}

// floats of one [rows, d] edge buffer per patch: only the unfused blocks materialise edge tensors; buffer 1 also holds
// conv_final's [points, emb] output
static void fn_edge_floats_per_patch(const sapcu_model* m, int mp, int64_t& first, int64_t& others) {
    first = (int64_t)mp * m->emb;
    others = 0;
    for (int l = 0; l < 3; ++l) {
        if (fn_block_fused(m, l, mp)) continue;
        const int64_t e = (int64_t)mp * imin(m->kv[l], mp) * (128 << l);
        first = imax(first, e);
        others = imax(others, e);
    }
}

// bytes of chunk workspace per patch, the budget estimate that picks the chunk size (an input to the layout below, not derived from
// it: un-rounded, linear in the chunk size): the edge buffers dominate when a block runs unfused
static int64_t fn_bytes_per_patch(const sapcu_model* m, int mp) {
    int64_t e1, e23;
    fn_edge_floats_per_patch(m, mp, e1, e23);
    int64_t idxs = 0;
    for (int l = 0; l < 3; ++l) idxs += (int64_t)mp * imin(m->kv[l], mp) * 4;
    return (e1 + 2 * e23) * 4 + idxs + (int64_t)mp * fn_kmax(m, mp) * 24 + (int64_t)mp * (64 + 192 + 512 + 1536 + 512) * 4 +
           ((int64_t)m->emb + 2048 + 1024 + 512 + 256 + 3) * 4;
}

// patches per chunk: SAPCU_CHUNK when set, else as many as the workspace budget holds (a multiple of 64, at least 64)
static int64_t chunk_patches(const sapcu_model* m, int64_t b, int64_t bytes_per_patch) {
    int64_t cb = m->chunk;
    if (cb <= 0) {
        cb = m->ws_budget / (bytes_per_patch > 0 ? bytes_per_patch : 1);
        cb = cb < 64 ? 64 : (cb / 64) * 64;
    }
    if (cb > b) cb = b;
    return cb < 1 ? 1 : cb;
}

static FnPlan fn_plan(const sapcu_model* m, int64_t b, int mp) {
    FnPlan pl;
    pl.cb = chunk_patches(m, b, fn_bytes_per_patch(m, mp));
    for (int l = 0; l < 3; ++l) pl.kk[l] = imin(m->kv[l], mp);
    pl.kmx = fn_kmax(m, mp);
    int64_t e1, e23;
    fn_edge_floats_per_patch(m, mp, e1, e23);
    pl.edge_floats = e1 * pl.cb;
    pl.edge_floats23 = e23 * pl.cb;
    return pl;
}

// The chunk workspace of fn_forward, every chunk in the same place.  base = the caller's pointer aligned up to 256 bytes, or null for
// the size alone (sapcu_workspace_bytes adds the 256 bytes the align-up may cost).
struct FnWs {
    int32_t* idx[3];         // [P, kk[l]] in-patch neighbour tables
    int2* tab;               // [P * kmx] edge table
    float4* pdiff;           // [P * kmx] position differences
    float *feat0, *cat, *X, *QKV, *RES;      // [P, 64 | 192 | 512 | 1536 | 512]
    float* B1;               // edge buffer 1; also conv_final's [P, emb] output, or its max keys [cb, emb] at the head
    float *B2, *B3;          // edge buffers 2, 3 (unfused blocks only)
    float *pooled, *enc, *h1, *h2, *h3, *logits;     // [cb, emb | 2048 | 1024 | 512 | 256 | 3]
    size_t bytes;
};

static FnWs fn_ws_layout(void* base, const sapcu_model* m, const FnPlan& pl, int mp) {
    const int64_t P = pl.cb * mp;
    WsCarver c(base);
    FnWs w;
    for (int l = 0; l < 3; ++l) w.idx[l] = c.take<int32_t>(P * pl.kk[l]);
    w.tab = c.take<int2>(P * pl.kmx);
    w.pdiff = c.take<float4>(P * pl.kmx);
    w.feat0 = c.take<float>(P * 64);
    w.cat = c.take<float>(P * 192);
    w.X = c.take<float>(P * 512);
    w.QKV = c.take<float>(P * 1536);
    w.RES = c.take<float>(P * 512);
    w.B1 = c.take<float>(pl.edge_floats);
    w.B2 = c.take<float>(pl.edge_floats23);
    w.B3 = c.take<float>(pl.edge_floats23);
    w.pooled = c.take<float>(pl.cb * m->emb);
    w.enc = c.take<float>(pl.cb * 2048);
    w.h1 = c.take<float>(pl.cb * 1024);
    w.h2 = c.take<float>(pl.cb * 512);
    w.h3 = c.take<float>(pl.cb * 256);
    w.logits = c.take<float>(pl.cb * 3);
    w.bytes = c.bytes();
    return w;
}

// offset (halves) inside chain_w of matrix q (0 fc_delta2, 1 fc_gamma, 2 fc_gamma2) of block l: the blocks in order, each three
// d x d matrices of hi | lo pairs in MFMA-fragment order; (3, 0) is the size of the whole
static int64_t chain_w_off(int l, int q) {
    int64_t off = 0;
    for (int i = 0; i < l; ++i) off += (int64_t)3 * 2 * (128 << i) * (128 << i);
    return off + (int64_t)q * 2 * (128 << l) * (128 << l);
}

// one fn block's edge chain over a chunk of P points: QKV [P, 3d] -> RES [P, d] (SP: as split rows)
struct FnEdge {
    const float* pc;         // the chunk's patches
    int64_t P;
    int mp, l, d, kk, sb, SP;
    float sqrt_hd;
    int64_t b1_floats;       // size of W.B1 (FnPlan::edge_floats)
};

// the whole edge chain in one kernel, activations in LDS (fn_edge_chain.hip)      fn:355-389
static int fn_edge_chain_fused(const sapcu_model* m, const FnWs& W, const FnEdge& e, hipStream_t st) {
    const int d = e.d, sb = e.sb;
    ChainArgs ca{};
    ca.P = e.P; ca.m = e.mp; ca.qkv = W.QKV; ca.ldq = 3 * d;
    ca.wd = m->p(sb + B_DELTA_W); ca.bd = m->p(sb + B_DELTA_B); ca.lifd = m->p(sb + B_DELTA_LIF);
    const _Float16* cw = (const _Float16*)m->chain_w;
    ca.w1p = cw + chain_w_off(e.l, 0); ca.b1 = m->p(sb + B_DELTA2_B); ca.lif1 = m->p(sb + B_DELTA2_LIF);
    ca.w2p = cw + chain_w_off(e.l, 1); ca.b2 = m->p(sb + B_GAMMA_B); ca.lif2 = m->p(sb + B_GAMMA_LIF);
    ca.w3p = cw + chain_w_off(e.l, 2); ca.b3 = m->p(sb + B_GAMMA2_B);
    ca.inv_sqrt_hd = 1.0f / e.sqrt_hd;
    ca.res = W.RES; ca.res_split = e.SP; ca.T = 4; ca.wide_offsets = m->opt_chain_wide ? 1 : 0;
    ca.trim = m->opt_chain_trim ? 1 : 0;
    // d = 512, filled groups: the straddlers' logits go to W.X (consumed by the q|k|v GEMM, not written again before the chain has
    // run) and their t = v_j + pe to W.B1 (unused between the last unfused chain and conv_final) — where both hold
    // [P / 16][12][512] floats; else the plain grouping
    if (m->opt_chain_fill && d == 512 && e.kk == 12) {
        const int64_t need = (e.P / 16) * 12 * 512;
        if (need > 0 && need <= e.P * 512 && need <= e.b1_floats) {
            ca.fill_x = W.X;
            ca.fill_t = W.B1;
        }
    }
    return launch_fn_edge_chain(ca, e.pc, W.idx[e.l], d, e.kk, W.tab, W.pdiff, st);
}

// the same chain as five kernels over [R, d] edge tensors in HBM (R = P * kk rows)
static int fn_edge_chain_unfused(const sapcu_model* m, const FnWs& W, const FnEdge& e, hipStream_t st) {
    const int d = e.d, kk = e.kk, sb = e.sb, SP = e.SP;
    const int64_t R = e.P * kk;
    const int32_t* idx = W.idx[e.l];
    // pe1 = LIF(fc_delta(x_i - x_j))                                        fn:310,355-358
    SAPCU_TRY(launch_fn_pe1(e.pc, idx, R, e.mp, kk, d, m->p(sb + B_DELTA_W), m->p(sb + B_DELTA_B), m->p(sb + B_DELTA_LIF), 4, W.B1, SP,
                            st));
    // pe = LIF(fc_delta2(pe1)) -> B2, and in the same epilogue attn_in = q_i - k_j + pe -> B3   fn:360-368
    SAPCU_TRY(launch_edge_table(idx, R, e.mp, kk, W.tab, st));
    SAPCU_TRY(run_gemm(m, Gemm(W.B1, R, d, d, m->p(sb + B_DELTA2_W), d, m->p(sb + B_DELTA2_B), W.B2, d, EPI_LIF_ATTN)
                              .neuron(m->p(sb + B_DELTA2_LIF), 4).attn(W.B3, W.QKV, d, W.tab).split_in(SP).split_out2(SP), st));
    // g = LIF(fc_gamma(attn_in)) -> B1                                      fn:373-376
    SAPCU_TRY(run_gemm(m, Gemm(W.B3, R, d, d, m->p(sb + B_GAMMA_W), d, m->p(sb + B_GAMMA_B), W.B1, d, EPI_LIF)
                              .neuron(m->p(sb + B_GAMMA_LIF), 4).split_in(SP).split_out(SP), st));
    // a = fc_gamma2(g) -> B3                                                fn:378
    SAPCU_TRY(run_gemm(m, Gemm(W.B1, R, d, d, m->p(sb + B_GAMMA2_W), d, m->p(sb + B_GAMMA2_B), W.B3, d, EPI_BIAS).split_in(SP), st));
    // res = sum_j softmax_j(a / sqrt(hd)) * (v_j + pe)                      fn:379-389
    return launch_fn_softmax_agg(W.B3, W.B2, W.QKV + 2 * d, 3 * d, idx, e.P, e.mp, kk, d, e.sqrt_hd, W.RES, SP, st);
}

static int fn_forward(const sapcu_model* m, const float* patch, int64_t b, int mp, const int32_t* knn_in,
                      int32_t* knn_out, float* normals, void* ws, int64_t ws_bytes, void* const* taps,
                      hipStream_t st) {
    const FnPlan pl = fn_plan(m, b, mp);
    const FnWs W = fn_ws_layout(ws_align256(ws), m, pl, mp);
    SAPCU_TRY(check_workspace("fn_forward", ws_bytes, W.bytes));
    // offsets of the three tables inside knn_in / knn_out ([b,m,k0] | [b,m,k1] | [b,m,k2])
    int64_t tab_off[3];
    tab_off[0] = 0;
    tab_off[1] = b * mp * pl.kk[0];
    tab_off[2] = tab_off[1] + b * mp * pl.kk[1];

    for (int64_t s = 0; s < b; s += pl.cb) {
        const int64_t cb = (b - s) < pl.cb ? (b - s) : pl.cb;
        const int64_t P = cb * mp;
        const float* pc = patch + s * mp * 3;

        // in-patch neighbour tables: replayed (reference KNNCache) or computed from this chunk (one xyz
        // ranking per patch serves the three blocks' k values)
        if (!knn_in) SAPCU_TRY(launch_patch_knn_multi(pc, cb, (int64_t)mp * 3, mp, 3, 3, 3, pl.kk, W.idx, st));
        for (int l = 0; l < 3; ++l) {
            const int64_t cnt = P * pl.kk[l];
            if (knn_in)
                SAPCU_CHECK_HIP(hipMemcpyAsync(W.idx[l], knn_in + tab_off[l] + s * mp * pl.kk[l], cnt * 4,
                                               hipMemcpyDeviceToDevice, st));
            if (knn_out)
                SAPCU_CHECK_HIP(hipMemcpyAsync(knn_out + tab_off[l] + s * mp * pl.kk[l], W.idx[l], cnt * 4,
                                               hipMemcpyDeviceToDevice, st));
        }
        SAPCU_TRY(launch_fn_stem(pc, P, m->p(FN_STEM_W), m->p(FN_STEM_B), m->p(FN_STEM_LIF), m->T, W.feat0, st));
        SAPCU_TRY(tap_copy(taps, SAPCU_FN_TAP_STEM, s * mp * 64 * 4, W.feat0, P * 64 * 4, st));

        const float* fin = W.feat0;
        int ldin = 64;
        for (int l = 0; l < 3; ++l) {
            const int d = 128 << l;
            const int sb = FN_BLK0 + l * B_SLOTS;
            // Tensors that only feed another GEMM travel as split rows (SP) in split-f16 mode: their producer
            // writes f16 hi/lo halves and the consuming GEMM streams them by LDS-DMA (gemm_sf16_ring.hip).
            const int SP = m->sf16 ? 1 : 0;
            float* const out = W.cat + 64 * l;             // the block's 64 output columns
            // x = LIF(fc1(feat))                                                    fn:317-320
            SAPCU_TRY(run_gemm(m, Gemm(fin, P, 64, ldin, m->p(sb + B_FC1_W), d, m->p(sb + B_FC1_B), W.X, d, EPI_LIF)
                                      .neuron(m->p(sb + B_SNN1), 4).split_out(SP), st));
            // q|k|v = LIF(w_qs|w_ks|w_vs (x))                                       fn:322-335
            SAPCU_TRY(run_gemm(m, Gemm(W.X, P, d, d, m->p(sb + B_QKV_W), 3 * d, m->p(sb + B_QKV_B), W.QKV, 3 * d, EPI_LIF)
                                      .neuron(m->p(sb + B_QKV_LIF), 4).split_in(SP), st));
            const FnEdge e{pc, P, mp, l, d, pl.kk[l], sb, SP, (float)sqrt((double)(d / m->heads)), pl.edge_floats};
            SAPCU_TRY(fn_block_fused(m, l, mp) ? fn_edge_chain_fused(m, W, e, st) : fn_edge_chain_unfused(m, W, e, st));
            // out_proj, fc2 + residual                                              fn:393-394
            if (m->opt_fn_fold_out) {
                // the two layers folded into one at model build (fold_w / fold_b): res goes straight to the block's 64 output columns
                SAPCU_TRY(run_gemm(m, Gemm(W.RES, P, d, d, m->blob + m->fold_w[l], 64, m->blob + m->fold_b[l], out, 192, EPI_RESID)
                                          .residual(fin, ldin).split_in(SP), st));
            } else {
                SAPCU_TRY(run_gemm(m, Gemm(W.RES, P, d, d, m->p(sb + B_OUT_W), d, m->p(sb + B_OUT_B), W.X, d, EPI_BIAS)
                                          .split_in(SP).split_out(SP), st));
                SAPCU_TRY(run_gemm(m, Gemm(W.X, P, d, d, m->p(sb + B_FC2_W), 64, m->p(sb + B_FC2_B), out, 192, EPI_RESID)
                                          .residual(fin, ldin).split_in(SP), st));
            }
            if (taps && taps[SAPCU_FN_TAP_BLOCK1 + l]) {
                SAPCU_CHECK_HIP(hipMemcpy2DAsync((char*)taps[SAPCU_FN_TAP_BLOCK1 + l] + s * mp * 64 * 4, 64 * 4,
                                                 out, 192 * 4, 64 * 4, (size_t)P, hipMemcpyDeviceToDevice, st));
            }
            fin = out;
            ldin = 192;
        }
        // conv_final + LIF x T_enc, max over points, fc_out                          fn:465-475
        if (m->sf16 && m->opt_fn_maxfuse) {
            // the max over the patch's points inside the GEMM's epilogue (integer atomicMax on order-preserving keys, as fd's
            // multi_scale_conv): the [P, emb] activation is never written.  Keys live at the head of the unused B1 area.
            unsigned* const keys = reinterpret_cast<unsigned*>(W.B1);
            // whole patches per row group (M = 48): gemm_shortk.hip takes the max in registers and writes pooled itself
            const bool direct = m->opt_shortk && mp == 48;
            if (!direct) SAPCU_CHECK_HIP(hipMemsetAsync(keys, 0, (size_t)cb * m->emb * 4, st));
            SAPCU_TRY(run_gemm(m, Gemm(W.cat, P, 192, 192, m->p(FN_FINAL_W), m->emb, m->p(FN_FINAL_B), nullptr, m->emb, EPI_LIF_MAX)
                                      .neuron(m->p(FN_FINAL_LIF), m->T).max_rows(keys, mp, direct ? W.pooled : nullptr), st));
            if (!direct) SAPCU_TRY(launch_decode_max_keys(keys, cb * m->emb, W.pooled, st));
        } else {
            SAPCU_TRY(run_gemm(m, Gemm(W.cat, P, 192, 192, m->p(FN_FINAL_W), m->emb, m->p(FN_FINAL_B), W.B1, m->emb, EPI_LIF)
                                      .neuron(m->p(FN_FINAL_LIF), m->T), st));
            SAPCU_TRY(launch_rowgroup_max(W.B1, cb, mp, m->emb, W.pooled, st));
        }
        SAPCU_TRY(tap_copy(taps, SAPCU_FN_TAP_POOLED, s * m->emb * 4, W.pooled, cb * m->emb * 4, st));
        SAPCU_TRY(run_gemm(m, Gemm(W.pooled, cb, m->emb, m->emb, m->p(FN_FCOUT_W), 2048, m->p(FN_FCOUT_B), W.enc, 2048, EPI_BIAS), st));
        SAPCU_TRY(tap_copy(taps, SAPCU_FN_TAP_ENC, s * 2048 * 4, W.enc, cb * 2048 * 4, st));
        // decoder MLP (Linear+BN+GELU) x3, Linear(256,3), LayerNorm(3), normalize    fn:542-549
        SAPCU_TRY(run_gemm(m, Gemm(W.enc, cb, 2048, 2048, m->p(FN_MLP0_W), 1024, m->p(FN_MLP0_B), W.h1, 1024, EPI_GELU), st));
        SAPCU_TRY(run_gemm(m, Gemm(W.h1, cb, 1024, 1024, m->p(FN_MLP1_W), 512, m->p(FN_MLP1_B), W.h2, 512, EPI_GELU), st));
        SAPCU_TRY(run_gemm(m, Gemm(W.h2, cb, 512, 512, m->p(FN_MLP2_W), 256, m->p(FN_MLP2_B), W.h3, 256, EPI_GELU), st));
        SAPCU_TRY(launch_fn_tail(W.h3, cb, 256, m->p(FN_HEAD_W), m->p(FN_HEAD_B), m->p(FN_LN_W), m->p(FN_LN_B), W.logits,
                                 normals + s * 3, st));
        SAPCU_TRY(tap_copy(taps, SAPCU_FN_TAP_LOGITS, s * 3 * 4, W.logits, cb * 3 * 4, st));
    }
    return SAPCU_OK;
}

// ============================================================================ fd
struct FdPlan {
    int64_t cb;
    int kmax0, kk;             // largest scale k and the feature-space k, both clamped to the patch
    bool fused;                // the whole encoder in fd_encoder.hip: no per-point intermediates in the workspace
    bool x0path;               // per-stage front + fd_msc_kernel: x0 [P, 960] and ONE spike slab instead of T slabs (round 4)
    bool maxfuse;              // multi_scale_conv's max over points inside the GEMM: the [T*P, emb] aggregate is never written
    int64_t agg_rows(int mp) const { return maxfuse ? 1 : mp; }   // rows of the AGG area per (step, patch): keys only, or the aggregate
};

// does the encoder run as ONE LDS-resident kernel per patch (fd_encoder.hip)?  Same answer for the workspace plan and the forward.
static bool fd_encoder_fused(const sapcu_model* m, int mp) {
    return m->sf16 && m->opt_fd_fused && m->fde_w && m->fde_nprm && fd_encoder_ok(mp, m->nscale, m->emb, m->T);
}

// does the per-stage path hand x0 to fd_msc_kernel (multi_scale_conv with the spikes regenerated on the CU) instead of writing the
// spikes of all T steps for the big-tile GEMM?  Patches of more than 48 points (the reference's default is 100), every T.
static bool fd_x0_path(const sapcu_model* m, int mp) {
    return !fd_encoder_fused(m, mp) && m->sf16 && m->opt_fd_fused && m->opt_fd_x0 && m->opt_fd_maxfuse && m->opt_fd_split && m->fde_w &&
           m->fde_nprm && fd_msc_ok(mp, m->emb, m->T);
}

// the largest k over the scales, clamped to the patch (every scale's table is a prefix of the sorted top-kmax0 list)
static int fd_kmax0(const sapcu_model* m, int mp) {
    int kmax = 1;
    for (int i = 0; i < m->nscale; ++i) kmax = kmax > m->ks[i] ? kmax : m->ks[i];
    return imin(kmax, mp);
}

static FdPlan fd_plan(const sapcu_model* m, int64_t b, int mp) {
    FdPlan pl;
    pl.fused = fd_encoder_fused(m, mp);
    pl.x0path = fd_x0_path(m, mp);
    pl.maxfuse = m->sf16 && m->opt_fd_maxfuse;
    pl.kmax0 = fd_kmax0(m, mp);
    pl.kk = imin(m->k, mp);
    // bytes per patch, the budget estimate that picks the chunk size (an input to the layout below, not derived from it).  With the
    // fused encoder the intermediates never leave the CU: per patch only pooled [T, emb], the encoding and the decoder's rows
    int64_t per_patch = ((int64_t)(m->T + 1) * m->emb + 256 + 3 * 128 + 3 * 64 + 192 + 64) * 4;
    if (!pl.fused) {
        // per-stage intermediates: T x 960 spikes (+ the T x emb aggregate per point only when the max is NOT taken inside the GEMM) +
        // 960 + 1024 + block-0 features per point, neighbour tables
        const int64_t slabs = pl.x0path ? 2 : m->T;        // x0 path: the step-0 spike slab (split rows) + x0, whatever T
        per_patch = (int64_t)mp * ((slabs * 960 + 960 + 1024 + 64 * (m->nscale + 1)) * 4 + (int64_t)(pl.kmax0 + 3 * pl.kk) * 4) +
                    (int64_t)m->T * pl.agg_rows(mp) * m->emb * 4 + per_patch;
    }
    pl.cb = chunk_patches(m, b, per_patch);
    return pl;
}

// The chunk workspace of fd_forward, every chunk in the same place; base as for fn_ws_layout.  The per-point intermediates exist
// only on the per-stage path (pp: the fused encoder keeps them on the CU and their regions are empty).
struct FdWs {
    int32_t* idx0;           // [P, kmax0] xyz neighbours
    int32_t* idxb;           // [3][P, kk] feature-space neighbours of blocks 1..3
    float* E0;               // [P, 64 * nscale]
    float* FUSED;            // [P, 64]
    float* SPK;              // [T][P, 960] spikes (x0 path: one slab), f32 or split rows
    float* F0;               // [P, 960] step-0 spikes as f32 when SPK holds split rows
    float* AB;               // [P, 1024] factored EdgeConv products
    float* AGG;              // [T * P, emb] aggregate; maxfuse: the [T, cb, emb] max keys only
    float* X0;               // x0 path: [P, 960] pre-activations
    float *POOLED, *ENC;     // [T, cb, emb], [cb, emb]
    float *D1, *D2a, *D2b, *D2c, *D3a, *D3b, *D3c, *QKV, *ATT;      // decoder rows [cb, 256 | 128 x 3 | 64 x 3 | 192 | 64]
    size_t bytes;
};

static FdWs fd_ws_layout(void* base, const sapcu_model* m, const FdPlan& pl, int mp) {
    const int64_t cb = pl.cb, T = m->T, emb = m->emb;
    const int64_t P = pl.fused ? 0 : cb * mp;
    WsCarver c(base);
    FdWs w;
    w.idx0 = c.take<int32_t>(P * pl.kmax0);
    w.idxb = c.take<int32_t>(3 * P * pl.kk);
    w.E0 = c.take<float>(P * 64 * m->nscale);
    w.FUSED = c.take<float>(P * 64);
    w.SPK = c.take<float>((pl.x0path ? 1 : T) * P * 960);
    w.F0 = c.take<float>(P * 960);
    w.AB = c.take<float>(P * 1024);
    w.AGG = c.take<float>(pl.fused ? 0 : T * cb * pl.agg_rows(mp) * emb);
    w.X0 = c.take<float>(pl.x0path ? P * 960 : 0);
    w.POOLED = c.take<float>(T * cb * emb);
    w.ENC = c.take<float>(cb * emb);
    w.D1 = c.take<float>(cb * 256);
    w.D2a = c.take<float>(cb * 128);
    w.D2b = c.take<float>(cb * 128);
    w.D2c = c.take<float>(cb * 128);
    w.D3a = c.take<float>(cb * 64);
    w.D3b = c.take<float>(cb * 64);
    w.D3c = c.take<float>(cb * 64);
    w.QKV = c.take<float>(cb * 192);
    w.ATT = c.take<float>(cb * 64);
    w.bytes = c.bytes();
    return w;
}

// one chunk of an fd forward: patches [s, s + cb) of the b in the call
struct FdChunk {
    const float* pc;
    int64_t s, cb, b;
    int mp;
    const int32_t* knn_force;
    void* const* taps;
    int64_t P() const { return cb * mp; }
    float* tap(int which) const { return taps ? (float*)taps[which] : nullptr; }
    float* x0_tap() const { return tap(SAPCU_FD_TAP_X0) ? tap(SAPCU_FD_TAP_X0) + s * mp * 960 : nullptr; }    // this chunk's rows
};

static const int FD_CIN[4] = {0, 64, 128, 256}, FD_COUT[4] = {64, 128, 256, 512}, FD_COFF[4] = {0, 64, 192, 448};

// the whole encoder up to pooled [T, cb, emb] in ONE launch, one workgroup per patch (fd_encoder.hip)   fd:408-480
static int fd_encode_fused(const sapcu_model* m, const FdPlan& pl, const FdWs& W, const FdChunk& c, hipStream_t st) {
    FdEncArgs ea{};
    ea.patch = c.pc; ea.b = c.cb; ea.b_total = c.b; ea.s0 = c.s;
    ea.m = c.mp; ea.T = m->T; ea.kk = pl.kk; ea.kmax0 = pl.kmax0; ea.nscale = m->nscale; ea.emb = m->emb;
    for (int i = 0; i < 4; ++i) ea.ks[i] = i < m->nscale ? imin(m->ks[i], c.mp) : 0;
    ea.e0_w = m->p(FD_E0_W); ea.e0_b = m->p(FD_E0_B);
    const _Float16* fw = (const _Float16*)m->fde_w;
    ea.fuse_wp = fw + m->fde_off[0]; ea.fuse_b = m->p(FD_FUSE_B);
    for (int l = 0; l < 3; ++l) {
        ea.edge_wp[l] = fw + m->fde_off[1 + l];
        ea.shift[l] = m->p(FD_EDGE1_SHIFT + 3 * l);
    }
    ea.msc_wp = fw + m->fde_off[4]; ea.msc_b = m->p(FD_MSC_B);
    ea.nprm = m->fde_nprm;
    ea.pooled = W.POOLED;
    ea.knn_force = c.knn_force;
    ea.tap_knn = (int32_t*)c.tap(SAPCU_FD_TAP_KNN);
    ea.tap_fused0 = c.tap(SAPCU_FD_TAP_FUSED0);
    ea.tap_spikes = c.tap(SAPCU_FD_TAP_SPIKES);
    ea.tap_x0 = c.tap(SAPCU_FD_TAP_X0);
    ea.gate = m->gate_dev; ea.ovf = m->ovf_dev;
    return launch_fd_encoder(ea, st);
}

// multi_scale_conv as a GEMM over the T spike slabs with the max over the points in its epilogue (keys at the head of AGG)
static Gemm fd_msc_gemm(const sapcu_model* m, const FdWs& W, const FdChunk& c, bool split_spikes) {
    return Gemm(W.SPK, (int64_t)m->T * c.P(), 960, 960, m->p(FD_MSC_W), m->emb, m->p(FD_MSC_B), nullptr, m->emb, EPI_LRELU_MAX)
        .max_rows(reinterpret_cast<unsigned*>(W.AGG), c.mp).split_in(split_spikes);
}

// The per-stage front: block 0 (xyz kNN, EdgeConv x S, scale fusion, EIF over T steps, fd:411-444) and blocks 1..3 (feature-space
// kNN on the t = 0 spikes, factored EdgeConv, neuron, fd:447-474).  Leaves the 960-channel spikes in SPK (x0 path: x0 in X0 and
// step 0 only) and says in split_spikes whether SPK holds split rows.
static int fd_front(const sapcu_model* m, const FdPlan& pl, const FdWs& W, const FdChunk& c, bool& split_spikes, hipStream_t st) {
    const int T = m->T, mp = c.mp;
    const int64_t P = c.P(), cb = c.cb, s = c.s, b = c.b;
    void* const* taps = c.taps;
    // all scales are prefixes of the sorted top-kmax list
    SAPCU_TRY(launch_patch_knn(c.pc, cb, mp, 3, 3, pl.kmax0, W.idx0, st));
    SAPCU_TRY(launch_fd_edge0(c.pc, W.idx0, pl.kmax0, P, mp, m->nscale, m->ks_dev, m->p(FD_E0_W), m->p(FD_E0_B), W.E0, st));
    SAPCU_TRY(run_gemm(m, Gemm(W.E0, P, 64 * m->nscale, 64 * m->nscale, m->p(FD_FUSE_W), 64, m->p(FD_FUSE_B), W.FUSED, 64, EPI_LRELU), st));
    SAPCU_TRY(tap_copy(taps, SAPCU_FD_TAP_FUSED0, s * mp * 64 * 4, W.FUSED, P * 64 * 4, st));
    float* const X0T = c.x0_tap();
    if (X0T) SAPCU_CHECK_HIP(hipMemcpy2DAsync(X0T, 960 * 4, W.FUSED, 64 * 4, 64 * 4, (size_t)P, hipMemcpyDeviceToDevice, st));
    // multi_scale_conv's operand: split rows written by the neuron kernels themselves (the GEMM then streams them by LDS-DMA
    // on the big-tile kernel and takes the max over the points in its epilogue) whenever that kernel takes the shape; the
    // step-0 spikes also go to F0 as f32 for the next blocks' neighbour search and EdgeConv.  Otherwise (tiny batches,
    // SAPCU_GEMM=f32, SAPCU_FD_MAXFUSE=0 / SAPCU_FD_SPLIT=0, or a caller asking for the spike tap): f32 spikes for all steps.
    split_spikes = pl.x0path;                               // x0 path: ONE slab of step-0 split rows (the EdgeConv GEMMs' operand)
    if (!pl.x0path && pl.maxfuse && m->opt_fd_split && !c.tap(SAPCU_FD_TAP_SPIKES)) {
        GemmArgs g = fd_msc_gemm(m, W, c, true);
        const char* why;
        const bool have16 = attach_split_weights(m, g);
        split_spikes = gemm_route(g, have16, m->opt_bt, m->opt_shortk, &why) == launch_gemm_sf16_bt;     // (the ring kernel has no max-over-rows epilogue)
    }
    float* const SPKS = split_spikes ? W.SPK : nullptr;     // [T*P, 960] split rows (same buffer, other format)
    float* const SPK0 = split_spikes ? W.F0 : W.SPK;        // where the step-0 f32 spikes live ([P, 960] slab)
    float* const X0P = pl.x0path ? W.X0 : nullptr;          // the neuron kernels then write x0 and run step 0 only
    SAPCU_TRY(launch_fd_neuron(true, 0, W.FUSED, 64, nullptr, 0, mp, nullptr, P, 64, m->p(FD_SNN0), T, SPK0, 960, 0,
                               nullptr, m->gate_dev, st, SPKS, X0P));
    for (int l = 1; l <= 3; ++l) {
        const int cin = FD_CIN[l], cout = FD_COUT[l], coff = FD_COFF[l - 1];
        int32_t* idl = W.idxb + (int64_t)(l - 1) * pl.cb * mp * pl.kk;
        const float* F = SPK0 + coff;          // t = 0 slab, row stride 960
        if (c.knn_force) {
            SAPCU_CHECK_HIP(hipMemcpyAsync(idl, c.knn_force + ((int64_t)(l - 1) * b + s) * mp * pl.kk, P * pl.kk * 4,
                                           hipMemcpyDeviceToDevice, st));
        } else {
            SAPCU_TRY(launch_patch_knn_strided(F, cb, (int64_t)mp * 960, mp, cin, 960, pl.kk, idl, st));
        }
        if (c.tap(SAPCU_FD_TAP_KNN))
            SAPCU_CHECK_HIP(hipMemcpyAsync((int32_t*)taps[SAPCU_FD_TAP_KNN] + ((int64_t)(l - 1) * b + s) * mp * pl.kk,
                                           idl, P * pl.kk * 4, hipMemcpyDeviceToDevice, st));
        const int ew = FD_EDGE1_W + 3 * (l - 1);
        // the factored EdgeConv's GEMM reads the step-0 spikes as split rows when the neuron kernels wrote them (rows 0..P-1 of
        // SPKS, same pitch and column offsets as the f32 slab): the all-DMA kernels instead of the f32-operand one, same sums
        SAPCU_TRY(run_gemm(m, Gemm(split_spikes ? SPKS + coff : F, P, cin, 960, m->p(ew), 2 * cout, nullptr, W.AB, 2 * cout, EPI_BIAS)
                                  .split_in(split_spikes), st));
        SAPCU_TRY(launch_fd_neuron(l == 1, 1, W.AB, 2 * cout, idl, pl.kk, mp, m->p(ew + 1), P, cout, m->p(ew + 2), T, SPK0, 960,
                                   FD_COFF[l], nullptr, m->gate_dev, st, SPKS, X0P));
        if (X0T && !pl.x0path)
            SAPCU_TRY(launch_fd_pre(W.AB, 2 * cout, idl, pl.kk, mp, m->p(ew + 1), P, cout, X0T, 960, FD_COFF[l], st));
    }
    return SAPCU_OK;
}

// multi_scale_conv over all T steps + max over the points straight from x0: every spike regenerated on the CU (fd_msc_kernel)
static int fd_msc_from_x0(const sapcu_model* m, const FdWs& W, const FdChunk& c, hipStream_t st) {
    if (c.x0_tap()) SAPCU_CHECK_HIP(hipMemcpyAsync(c.x0_tap(), W.X0, (size_t)c.P() * 960 * 4, hipMemcpyDeviceToDevice, st));
    FdMscArgs ma{};
    ma.x0 = W.X0; ma.b = c.cb; ma.b_total = c.b; ma.s0 = c.s; ma.m = c.mp; ma.T = m->T; ma.emb = m->emb;
    ma.msc_wp = (const _Float16*)m->fde_w + m->fde_off[4]; ma.msc_b = m->p(FD_MSC_B); ma.nprm = m->fde_nprm;
    ma.pooled = W.POOLED; ma.tap_spikes = c.tap(SAPCU_FD_TAP_SPIKES); ma.gate = m->gate_dev;
    return launch_fd_msc(ma, st);
}

// multi_scale_conv + BN + LeakyReLU over all T*P rows of the spike slabs, max over points        fd:476-480
static int fd_msc_from_slabs(const sapcu_model* m, const FdPlan& pl, const FdWs& W, const FdChunk& c, bool split_spikes, hipStream_t st) {
    const int T = m->T, emb = m->emb;
    const int64_t P = c.P();
    SAPCU_TRY(tap_copy_steps(c.taps, SAPCU_FD_TAP_SPIKES, T, c.b, c.s, c.cb, (int64_t)c.mp * 960, W.SPK, st));
    if (pl.maxfuse) {
        // the max over the patch's points inside the GEMM's epilogue (integer atomicMax on order-preserving keys): the
        // [T*P, emb] aggregate is never written.  The key buffer is the head of the (otherwise unused) AGG area.
        const Gemm mg = fd_msc_gemm(m, W, c, split_spikes);
        SAPCU_CHECK_HIP(hipMemsetAsync(mg.max_keys, 0, (size_t)T * c.cb * emb * 4, st));
        SAPCU_TRY(run_gemm(m, mg, st));
        return launch_decode_max_keys(mg.max_keys, (int64_t)T * c.cb * emb, W.POOLED, st);
    }
    SAPCU_TRY(run_gemm(m, Gemm(W.SPK, (int64_t)T * P, 960, 960, m->p(FD_MSC_W), emb, m->p(FD_MSC_B), W.AGG, emb, EPI_LRELU), st));
    return launch_rowgroup_max(W.AGG, (int64_t)T * c.cb, c.mp, emb, W.POOLED, st);
}

// pooled [T, cb, emb] -> temporal integration -> decoder -> distances (every encoder path ends here)
static int fd_temporal_decoder(const sapcu_model* m, const FdWs& W, const FdChunk& c, float* dist, hipStream_t st) {
    const int T = m->T, emb = m->emb;
    const int64_t cb = c.cb, s = c.s;
    SAPCU_TRY(tap_copy_steps(c.taps, SAPCU_FD_TAP_POOLED, T, c.b, s, cb, emb, W.POOLED, st));
    SAPCU_TRY(launch_fd_temporal(W.POOLED, T, cb, emb, m->p(FD_TI_W), m->p(FD_SNNFC), W.ENC, st));
    SAPCU_TRY(tap_copy(c.taps, SAPCU_FD_TAP_ENC, s * emb * 4, W.ENC, cb * emb * 4, st));
    // decoder                                                                    fd:711-725
    SAPCU_TRY(run_gemm(m, Gemm(W.ENC, cb, emb, emb, m->p(FD_FCIN_W), 256, m->p(FD_FCIN_B), W.D1, 256, EPI_GELU), st));
    SAPCU_TRY(run_gemm(m, Gemm(W.D1, cb, 256, 256, m->p(FD_R0_FC0_W), 128, m->p(FD_R0_FC0_B), W.D2a, 128, EPI_GELU), st));
    SAPCU_TRY(run_gemm(m, Gemm(W.D1, cb, 256, 256, m->p(FD_R0_PROJ_W), 128, m->p(FD_R0_PROJ_B), W.D2b, 128, EPI_BIAS), st));
    SAPCU_TRY(run_gemm(m, Gemm(W.D2a, cb, 128, 128, m->p(FD_R0_FC4_W), 128, m->p(FD_R0_FC4_B), W.D2c, 128, EPI_RESID_GELU).residual(W.D2b, 128),
                       st));
    SAPCU_TRY(run_gemm(m, Gemm(W.D2c, cb, 128, 128, m->p(FD_R1_FC0_W), 64, m->p(FD_R1_FC0_B), W.D3a, 64, EPI_GELU), st));
    SAPCU_TRY(run_gemm(m, Gemm(W.D2c, cb, 128, 128, m->p(FD_R1_PROJ_W), 64, m->p(FD_R1_PROJ_B), W.D3b, 64, EPI_BIAS), st));
    SAPCU_TRY(run_gemm(m, Gemm(W.D3a, cb, 64, 64, m->p(FD_R1_FC4_W), 64, m->p(FD_R1_FC4_B), W.D3c, 64, EPI_RESID_GELU).residual(W.D3b, 64), st));
    SAPCU_TRY(run_gemm(m, Gemm(W.D3c, cb, 64, 64, m->p(FD_QKV_W), 192, m->p(FD_QKV_B), W.QKV, 192, EPI_BIAS), st));
    return launch_fd_tail(W.D3c, W.QKV, cb, m->heads, m->p(FD_WO_T), m->p(FD_BO), m->p(FD_LN_W), m->p(FD_LN_B), m->p(FD_WH_T),
                          m->p(FD_BH), m->p(FD_WD), m->p(FD_BD), W.ATT, dist + s, st);
}

static int fd_forward(const sapcu_model* m, const float* patch, int64_t b, int mp, const int32_t* knn_force,
                      float* dist, void* ws, int64_t ws_bytes, void* const* taps, hipStream_t st) {
    const FdPlan pl = fd_plan(m, b, mp);
    const FdWs W = fd_ws_layout(ws_align256(ws), m, pl, mp);
    SAPCU_TRY(check_workspace("fd_forward", ws_bytes, W.bytes));
    for (int64_t s = 0; s < b; s += pl.cb) {
        const FdChunk c{patch + s * mp * 3, s, (b - s) < pl.cb ? (b - s) : pl.cb, b, mp, knn_force, taps};
        if (pl.fused) {
            SAPCU_TRY(fd_encode_fused(m, pl, W, c, st));
        } else {
            bool split_spikes = false;
            SAPCU_TRY(fd_front(m, pl, W, c, split_spikes, st));
            SAPCU_TRY(pl.x0path ? fd_msc_from_x0(m, W, c, st) : fd_msc_from_slabs(m, pl, W, c, split_spikes, st));
        }
        SAPCU_TRY(fd_temporal_decoder(m, W, c, dist, st));
    }
    return SAPCU_OK;
}

}  // namespace sapcu

// ================================================================================== C ABI
using namespace sapcu;

extern "C" {

int sapcu_abi_version(void) { return SAPCU_ABI_VERSION; }
const char* sapcu_last_error(void) { return g_err; }

int sapcu_knn_gather_f64(const double* cloud, int64_t n, const double* queries, int64_t b, int k, int64_t* idx_out,
                         double* dist_out, float* patch_out, void* stream) {
    SAPCU_CHECK_ARG(cloud && queries && idx_out, "knn_gather: null pointer");
    SAPCU_CHECK_ARG(n >= 1 && b >= 0 && k >= 1 && k <= 128 && k <= n, "knn_gather: need 1 <= k <= min(128, n) (n=%lld k=%d)",
                    (long long)n, k);
    SAPCU_CHECK_ARG(n < 0x7fffffffLL, "knn_gather: n too large");
    return launch_knn_outer(cloud, n, queries, b, k, idx_out, dist_out, patch_out, (hipStream_t)stream);
}

int sapcu_gather_rotate_f64(const double* cloud, int64_t n, const double* queries, int64_t b, const int64_t* idx, int k,
                            const float* normals, float* patch_out, void* stream) {
    SAPCU_CHECK_ARG(cloud && queries && idx && patch_out, "gather_rotate: null pointer");
    SAPCU_CHECK_ARG(n >= 1 && b >= 0 && k >= 1, "gather_rotate: bad sizes");
    return launch_gather_rotate(cloud, n, queries, b, idx, k, normals, patch_out, (hipStream_t)stream);
}

int sapcu_displace_f64(const double* queries, const float* normals, const float* dist, int64_t b, double* out,
                       void* stream) {
    SAPCU_CHECK_ARG(queries && normals && dist && out && b >= 0, "displace: bad argument");
    return launch_displace(queries, normals, dist, b, out, (hipStream_t)stream);
}

int64_t sapcu_fps_workspace_bytes(int64_t npoint) { return npoint < 0 ? -1 : (int64_t)fps_workspace_bytes((int)npoint); }

int sapcu_fps_f32(const float* xyz, int64_t n, int64_t npoint, int64_t* idx_out, void* workspace, int64_t workspace_bytes,
                  void* stream) {
    SAPCU_CHECK_ARG(npoint >= 0 && npoint <= n && n < (int64_t)1 << 31, "fps: need 0 <= npoint <= n < 2^31 (n=%lld npoint=%lld)",
                    (long long)n, (long long)npoint);
    if (npoint == 0) return SAPCU_OK;
    SAPCU_CHECK_ARG(xyz && idx_out && workspace, "fps: null pointer");
    SAPCU_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "fps: the workspace must be 8-byte aligned (64-bit mailboxes)");
    if (workspace_bytes < (int64_t)fps_workspace_bytes((int)npoint)) {
        set_error("fps: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
                  (long long)fps_workspace_bytes((int)npoint));
        return SAPCU_ERR_WORKSPACE;
    }
    int rc = launch_fps(xyz, n, (int)npoint, (int)(n / 2), idx_out, workspace, (hipStream_t)stream);
    if (rc != SAPCU_OK) return rc;
    SAPCU_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    int flag = 0;
    rc = fps_failed(workspace, (int)npoint, &flag);
    if (rc != SAPCU_OK) return rc;
    if (flag) {
        set_error("fps: a workgroup of the persistent grid never arrived at the step barrier (grid not resident)");
        return SAPCU_ERR_HIP;
    }
    return SAPCU_OK;
}

int sapcu_neuron_selfloop(const float* x, int64_t rows, int channels, int steps, const float* membrane_decay,
                          const float* threshold_adapt, const float* refractory_decay, const float* threshold_base,
                          const float* delta_T, const float* theta_rh, float* spikes_out, float* membrane_out,
                          float* threshold_out, float* refractory_out, void* stream) {
    SAPCU_CHECK_ARG(x && membrane_decay && threshold_adapt && refractory_decay && threshold_base, "neuron: null pointer");
    SAPCU_CHECK_ARG((delta_T == nullptr) == (theta_rh == nullptr), "neuron: delta_T and theta_rh go together");
    SAPCU_CHECK_ARG(rows >= 0 && channels >= 1 && steps >= 1, "neuron: bad sizes");
    return launch_neuron_selfloop(x, rows, channels, steps, membrane_decay, threshold_adapt, refractory_decay,
                                  threshold_base, delta_T, theta_rh, spikes_out, membrane_out, threshold_out,
                                  refractory_out, (hipStream_t)stream);
}

int sapcu_neuron_drive(const float* x, int64_t rows, int channels, int steps, const float* membrane_decay,
                       const float* threshold_adapt, const float* refractory_decay, const float* threshold_base,
                       const float* delta_T, const float* theta_rh, int channel_pairs, float* spikes_out, float* membrane_out,
                       float* threshold_out, float* refractory_out, int* gate_open_out, void* stream) {
    SAPCU_CHECK_ARG(x && membrane_decay && threshold_adapt && refractory_decay && threshold_base, "neuron_drive: null pointer");
    SAPCU_CHECK_ARG((delta_T == nullptr) == (theta_rh == nullptr), "neuron_drive: delta_T and theta_rh go together");
    SAPCU_CHECK_ARG(rows >= 0 && channels >= 1 && steps >= 1, "neuron_drive: bad sizes");
    return launch_neuron_drive(x, rows, channels, steps, membrane_decay, threshold_adapt, refractory_decay, threshold_base, delta_T,
                               theta_rh, channel_pairs, spikes_out, membrane_out, threshold_out, refractory_out, gate_open_out,
                               (hipStream_t)stream);
}

int sapcu_patch_knn(const float* feat, int64_t b, int m, int c, int ld, int k, int32_t* idx_out, void* stream) {
    SAPCU_CHECK_ARG(feat && idx_out && b >= 0 && ld >= c, "patch_knn: bad argument");
    return launch_patch_knn(feat, b, m, c, ld, k, idx_out, (hipStream_t)stream);
}

int sapcu_l2_normalize3(const float* in, float* out, int64_t b, void* stream) {
    SAPCU_CHECK_ARG(in && out && b >= 0, "l2_normalize3: bad argument");
    return launch_l2_normalize3(in, out, b, (hipStream_t)stream);
}

int sapcu_gemm_f32(const float* a, int64_t r, int k, int lda, const float* w, int n, const float* bias,
                   const float* lif4, int lif_steps, float* c, int ldc, void* w16_ws, int a_split_rows, int c_split_rows,
                   void* stream) {
    SAPCU_CHECK_ARG(a && w && c && r >= 0 && n >= 1, "gemm: bad argument");
    SAPCU_CHECK_ARG(!lif4 || lif_steps >= 1, "gemm: lif_steps must be >= 1");
    SAPCU_CHECK_ARG(!(a_split_rows || c_split_rows) || w16_ws, "gemm: split rows need the split-f16 kernels (w16_ws)");
    // the documented contract (include/sapcu.h), checked here for every kernel: the launchers below check what their own loads need
    SAPCU_CHECK_ARG(r == 0 || (k > 0 && k % 32 == 0 && lda >= k && ldc >= n), "gemm: need k %% 32 == 0, lda >= k and ldc >= n (k=%d lda=%d n=%d ldc=%d)", k, lda, n, ldc);
    SAPCU_CHECK_ARG(r == 0 || ((((uintptr_t)a | (uintptr_t)w | (uintptr_t)w16_ws) & 15) == 0 && lda % (a_split_rows ? 8 : 4) == 0),
                    "gemm: A, W and w16_ws must be 16-byte aligned, lda %% 4 == 0 (%% 8 for split rows) (lda=%d)", lda);
    Gemm g(a, r, k, lda, w, n, bias, c, ldc, lif4 ? EPI_LIF : EPI_BIAS);
    g.neuron(lif4, lif_steps).split_in(a_split_rows != 0).split_out(c_split_rows != 0);
    // a_split_rows = 2: the ring kernel even where the big-tile kernel takes the shape (bit-identical; parity tests)
    const SplitWs sw(w16_ws, (int64_t)n * k);
    if (w16_ws) sw.attach(g);
    return gemm_run(g, w16_ws != nullptr, a_split_rows != 2, !env_is("SAPCU_SHORTK", "0"), (hipStream_t)stream, &sw);
}

int sapcu_to_split_rows(const float* in, int64_t rows, int k, int ld_in, float* out, int ld_out, void* stream) {
    SAPCU_CHECK_ARG(in && out && rows >= 0 && k >= 1 && ld_in >= k && ld_out >= k, "to_split_rows: bad argument");
    return launch_to_split_rows(in, rows, k, ld_in, out, ld_out, (hipStream_t)stream);
}

int sapcu_posenc_gemm_f32(const float* pe1, int64_t r, int d, const float* w, const float* bias, const float* lif4,
                          int lif_steps, const float* qkv, const int32_t* idx, int kk, int m_pts, float* pe_out,
                          float* attn_in_out, void* edge_table_ws, void* w16_ws, int split_rows, void* stream) {
    SAPCU_CHECK_ARG(pe1 && w && lif4 && qkv && idx && pe_out && attn_in_out && edge_table_ws && r >= 0 && d >= 32 &&
                        lif_steps >= 1 && kk >= 1 && m_pts >= 1,
                    "posenc_gemm: bad argument");
    // every refusal comes before the first launch (the edge table below is already a kernel that writes edge_table_ws)
    SAPCU_CHECK_ARG(!split_rows || w16_ws, "posenc_gemm: split rows need the split-f16 kernels (w16_ws)");
    SAPCU_CHECK_ARG(d % 32 == 0, "posenc_gemm: d=%d must be a multiple of 32", d);
    SAPCU_CHECK_ARG((((uintptr_t)pe1 | (uintptr_t)w | (uintptr_t)w16_ws) & 15) == 0 && ((uintptr_t)edge_table_ws & 7) == 0,
                    "posenc_gemm: pe1, w and w16_ws must be 16-byte aligned, edge_table_ws 8-byte aligned");
    // split_rows: the production form, pe1 arrives as split rows and attn_in leaves as split rows; 2: ring kernel only
    Gemm g(pe1, r, d, d, w, d, bias, pe_out, d, EPI_LIF_ATTN);
    g.neuron(lif4, lif_steps).attn(attn_in_out, qkv, d, (const int2*)edge_table_ws).split_in(split_rows != 0).split_out2(split_rows != 0);
    const SplitWs sw(w16_ws, (int64_t)d * d);
    if (w16_ws) sw.attach(g);
    const char* why = nullptr;      // the route asked once more up here: its refusals, too, come before the edge table is written
    SAPCU_CHECK_ARG(gemm_route(g, w16_ws != nullptr, split_rows != 2, false, &why), "%s", why);
    SAPCU_TRY(launch_edge_table(idx, r, m_pts, kk, (int2*)edge_table_ws, (hipStream_t)stream));
    return gemm_run(g, w16_ws != nullptr, split_rows != 2, false, (hipStream_t)stream, &sw);
}

// workspace of sapcu_fn_edge_chain_f32 (base: the caller's pointer aligned up, or null for the size; the sizer adds 256 bytes)
struct ChainWs {
    int2* tab;               // [points * kk] edge table
    float4* pd;              // [points * kk] position differences
    char* split[3];          // per matrix: hi | lo | overflow counter
    _Float16* packed[3];     // per matrix: MFMA-fragment order
    size_t bytes;
};

static ChainWs chain_ws_layout(void* base, int64_t points, int d, int kk) {
    WsCarver c(base);
    ChainWs w;
    w.tab = c.take<int2>(points * kk);
    w.pd = c.take<float4>(points * kk);
    for (int q = 0; q < 3; ++q) {
        w.split[q] = c.take<char>((int64_t)d * d * 4 + 16);
        w.packed[q] = c.take<_Float16>((int64_t)d * d * 2);
    }
    w.bytes = c.bytes();
    return w;
}

int64_t sapcu_fn_edge_chain_workspace_bytes(int64_t points, int d, int kk) {
    if (points < 0 || !fn_edge_chain_ok(d, kk)) {
        set_error("fn_edge_chain_workspace_bytes: unsupported shape (d=%d kk=%d)", d, kk);
        return SAPCU_ERR_ARG;
    }
    return (int64_t)chain_ws_layout(nullptr, points, d, kk).bytes + 256;
}

int sapcu_fn_edge_chain_f32(const float* patch, const int32_t* idx, int64_t points, int m_pts, int d, int kk,
                            const float* qkv, const float* w_delta, const float* b_delta, const float* lif_delta,
                            const float* w1, const float* b1, const float* lif1, const float* w2, const float* b2,
                            const float* lif2, const float* w3, const float* b3, int heads, int lif_steps,
                            float* res_out, void* workspace, int64_t workspace_bytes, void* stream) {
    SAPCU_CHECK_ARG(patch && idx && qkv && w_delta && b_delta && lif_delta && w1 && b1 && lif1 && w2 && b2 && lif2 && w3 && b3 &&
                        res_out && workspace, "fn_edge_chain: null pointer");
    SAPCU_CHECK_ARG(fn_edge_chain_ok(d, kk), "fn_edge_chain: unsupported shape (d=%d kk=%d)", d, kk);
    SAPCU_CHECK_ARG(points >= 0 && m_pts >= kk && heads >= 1 && d % heads == 0 && lif_steps >= 1, "fn_edge_chain: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    const ChainWs W = chain_ws_layout(ws_align256(workspace), points, d, kk);
    SAPCU_TRY(check_workspace("fn_edge_chain", workspace_bytes, W.bytes));
    const float* ws[3] = {w1, w2, w3};
    for (int q = 0; q < 3; ++q) {
        const SplitWs sw(W.split[q], (int64_t)d * d);
        SAPCU_TRY(sw.fill(ws[q], st));
        SAPCU_TRY(launch_pack_chain_weights(sw.hi, sw.lo, d, W.packed[q], st));
    }
    ChainArgs ca{};
    ca.P = points; ca.m = m_pts; ca.qkv = qkv; ca.ldq = 3 * d;
    ca.wd = w_delta; ca.bd = b_delta; ca.lifd = lif_delta;
    ca.w1p = W.packed[0]; ca.b1 = b1; ca.lif1 = lif1;
    ca.w2p = W.packed[1]; ca.b2 = b2; ca.lif2 = lif2;
    ca.w3p = W.packed[2]; ca.b3 = b3;
    ca.inv_sqrt_hd = 1.0f / (float)sqrt((double)(d / heads));
    ca.res = res_out; ca.res_split = 0; ca.T = lif_steps;
    ca.trim = 1;
#ifdef CHAIN_STAMPS
    // diagnostic build (profiles/chain_stamps.py): the stamps go behind what the entry needs, where the caller's workspace has the room
    // (16 slots of 8 bytes per group, at most points / 4 + 1 groups), and SAPCU_CHAIN_TRIM=0 is honoured at every call
    {
        const int64_t sbytes = (points / 4 + 1) * 16 * 8;
        const int64_t off = ((int64_t)W.bytes + 256 + 255) / 256 * 256;
        if (workspace_bytes >= off + sbytes + 256) ca.stamps = (unsigned long long*)((char*)ws_align256(workspace) + off);
        if (env_is("SAPCU_CHAIN_TRIM", "0")) ca.trim = 0;
    }
#endif
    return launch_fn_edge_chain(ca, patch, idx, d, kk, W.tab, W.pd, st);
}

// ---- sapcu_model_create, stage by stage: each returns a status; the handle under construction frees itself on any failure
static int parse_fn_hparams(sapcu_model* m, const int32_t* hp, int n_hp, int n_dir) {
    SAPCU_CHECK_ARG(n_hp == 6 && n_dir == FN_SLOTS, "model_create(fn): need 6 hparams and %d slots (got %d, %d)", (int)FN_SLOTS, n_hp, n_dir);
    m->kv[0] = hp[0]; m->kv[1] = hp[1]; m->kv[2] = hp[2];
    m->emb = hp[3]; m->T = hp[4]; m->heads = hp[5];
    SAPCU_CHECK_ARG(m->kv[0] >= 1 && m->kv[1] >= 1 && m->kv[2] >= 1 && m->emb >= 32 && m->emb % 32 == 0 && m->T >= 1 && m->heads >= 1 &&
                        128 % m->heads == 0,
                    "model_create(fn): unsupported hyper-parameters");
    return SAPCU_OK;
}

static int parse_fd_hparams(sapcu_model* m, const int32_t* hp, int n_hp, int n_dir) {
    SAPCU_CHECK_ARG(n_hp >= 6 && n_dir == FD_SLOTS && hp[4] >= 1 && hp[4] <= 8 && n_hp == 5 + hp[4],
                    "model_create(fd): need [k,emb,T,heads,S,ks...] and %d slots", (int)FD_SLOTS);
    m->k = hp[0]; m->emb = hp[1]; m->T = hp[2]; m->heads = hp[3]; m->nscale = hp[4];
    for (int i = 0; i < m->nscale; ++i) m->ks[i] = hp[5 + i];
    SAPCU_CHECK_ARG(m->k >= 1 && m->emb >= 32 && m->emb % 32 == 0 && m->T >= 1 && m->T <= 64, "model_create(fd): unsupported hyper-parameters");
    // the decoder's attention splits 64 channels into heads on the lanes of one wave (launch_fd_tail checks it again)
    SAPCU_CHECK_ARG(m->heads >= 1 && m->heads <= 64 && (m->heads & (m->heads - 1)) == 0,
                    "model_create(fd): num_heads must be a power of two <= 64 (got %d)", m->heads);
    for (int i = 0; i < m->nscale; ++i) SAPCU_CHECK_ARG(m->ks[i] >= 1, "model_create(fd): k_scales[%d] = %d, need >= 1", i, m->ks[i]);
    return SAPCU_OK;
}

static int check_slot_directory(sapcu_model* m, const int64_t* dir_host, int n_dir, int64_t blob_floats) {
    m->dir.assign(dir_host, dir_host + n_dir);
    for (int i = 0; i < n_dir; ++i)
        SAPCU_CHECK_ARG(m->dir[i] >= 0 && m->dir[i] < blob_floats && (m->dir[i] & 3) == 0,
                        "model_create: slot %d offset %lld out of range / unaligned", i, (long long)m->dir[i]);
    return SAPCU_OK;
}

// the caller's blob on the device and, for fn with the fold on, W' [64, d] | b' [64] of the three blocks behind it (256-byte aligned pieces)
static int copy_blob_and_fold(sapcu_model* m, const float* blob, int64_t blob_floats) {
    int64_t total = blob_floats;
    if (m->kind == SAPCU_KIND_FN && m->opt_fn_fold_out) {
        total = (total + 63) & ~(int64_t)63;
        for (int l = 0; l < 3; ++l) {
            m->fold_w[l] = total;
            total += (int64_t)64 * (128 << l);
            m->fold_b[l] = total;
            total += 64;
        }
    }
    m->blob_floats = total;
    SAPCU_CHECK_HIP(hipMalloc((void**)&m->blob, (size_t)total * 4));
    SAPCU_CHECK_HIP(hipMemcpy(m->blob, blob, (size_t)blob_floats * 4, hipMemcpyDeviceToDevice));
    if (total == blob_floats) return SAPCU_OK;
    SAPCU_CHECK_HIP(hipMemset(m->blob + blob_floats, 0, (size_t)(total - blob_floats) * 4));
    for (int l = 0; l < 3; ++l) {
        // W' = W_fc2 . W_out, b' = W_fc2 . b_out + b_fc2 on the host in f64 (once per model), before the weights are split
        const int d = 128 << l, sb = FN_BLK0 + l * B_SLOTS;
        const int64_t need[4] = {(int64_t)d * d, d, (int64_t)64 * d, 64};
        static const int slot[4] = {B_OUT_W, B_OUT_B, B_FC2_W, B_FC2_B};
        std::vector<float> h[4], wf((size_t)64 * d), bf(64);
        for (int q = 0; q < 4; ++q) {
            SAPCU_CHECK_ARG(m->dir[sb + slot[q]] + need[q] <= blob_floats, "model_create(fn): slot %d runs past the end of the blob", sb + slot[q]);
            h[q].resize((size_t)need[q]);
            SAPCU_CHECK_HIP(hipMemcpy(h[q].data(), m->p(sb + slot[q]), (size_t)need[q] * 4, hipMemcpyDeviceToHost));
        }
        fold_affine_f64(h[0].data(), h[1].data(), h[2].data(), h[3].data(), d, 64, wf.data(), bf.data());
        SAPCU_CHECK_HIP(hipMemcpy(m->blob + m->fold_w[l], wf.data(), wf.size() * 4, hipMemcpyHostToDevice));
        SAPCU_CHECK_HIP(hipMemcpy(m->blob + m->fold_b[l], bf.data(), bf.size() * 4, hipMemcpyHostToDevice));
    }
    return SAPCU_OK;
}

// the overflow counters; in split-f16 mode the whole blob as f16 hi / lo planes — a parameter beyond the f16 range: exact-f32 kernels
static int split_blob_f16(sapcu_model* m) {
    SAPCU_CHECK_HIP(hipMalloc((void**)&m->ovf_dev, 2 * sizeof(int)));
    SAPCU_CHECK_HIP(hipMemset(m->ovf_dev, 0, 2 * sizeof(int)));
    if (!m->sf16) return SAPCU_OK;
    SAPCU_CHECK_HIP(hipMalloc(&m->w16_hi, (size_t)m->blob_floats * 2));
    SAPCU_CHECK_HIP(hipMalloc(&m->w16_lo, (size_t)m->blob_floats * 2));
    int wovf = 0;
    SAPCU_TRY(launch_split_weights(m->blob, m->blob_floats, m->w16_hi, m->w16_lo, m->ovf_dev + 1, nullptr));
    SAPCU_CHECK_HIP(hipMemcpy(&wovf, m->ovf_dev + 1, sizeof(int), hipMemcpyDeviceToHost));
    if (wovf != 0) m->sf16 = false;
    return SAPCU_OK;
}

// fn blocks 1-3 (d = 128, 256, 512): the three d x d matrices of the edge chain again in MFMA-fragment order
static int pack_fn_chain_weights(sapcu_model* m) {
    if (!m->sf16 || m->kind != SAPCU_KIND_FN) return SAPCU_OK;
    SAPCU_CHECK_HIP(hipMalloc(&m->chain_w, (size_t)chain_w_off(3, 0) * 2));
    for (int l = 0; l < 3; ++l) {
        static const int slots[3] = {B_DELTA2_W, B_GAMMA_W, B_GAMMA2_W};
        for (int q = 0; q < 3; ++q) {
            const int64_t wo = m->dir[FN_BLK0 + l * B_SLOTS + slots[q]];
            SAPCU_TRY(launch_pack_chain_weights((const _Float16*)m->w16_hi + wo, (const _Float16*)m->w16_lo + wo, 128 << l,
                                                (_Float16*)m->chain_w + chain_w_off(l, q), nullptr));
        }
    }
    SAPCU_CHECK_HIP(hipDeviceSynchronize());
    return SAPCU_OK;
}

// fd: the scale table and the gate counter; the fused encoder's operands — five matrices in fragment order (hi | lo planes interleaved
// per fragment), neuron parameters clamped once.  More than four scales: the fused encoder does not take the model, fd_msc_kernel (the
// x0 path) does — it reads multi_scale_conv and the neuron parameters only, so the first four matrices stay out (first = 4)
static int pack_fd_encoder(sapcu_model* m) {
    if (m->kind != SAPCU_KIND_FD) return SAPCU_OK;
    SAPCU_CHECK_HIP(hipMalloc((void**)&m->ks_dev, 8 * sizeof(int32_t)));
    SAPCU_CHECK_HIP(hipMemcpy(m->ks_dev, m->ks, 8 * sizeof(int32_t), hipMemcpyHostToDevice));
    SAPCU_CHECK_HIP(hipMalloc((void**)&m->gate_dev, sizeof(int)));
    SAPCU_CHECK_HIP(hipMemset(m->gate_dev, 0, sizeof(int)));
    if (!m->sf16 || m->emb < 96) return SAPCU_OK;
    const int first = m->nscale <= 4 ? 0 : 4;
    const int mats[5][3] = {{FD_FUSE_W, 64, 64 * m->nscale}, {FD_EDGE1_W, 256, 64}, {FD_EDGE2_W, 512, 128},
                            {FD_EDGE3_W, 1024, 256}, {FD_MSC_W, m->emb, 960}};
    int64_t halves = 0;
    for (int i = 0; i < 5; ++i) {
        m->fde_off[i] = halves;
        if (i >= first) halves += (int64_t)2 * mats[i][1] * mats[i][2];
    }
    SAPCU_CHECK_HIP(hipMalloc(&m->fde_w, (size_t)halves * 2));
    SAPCU_CHECK_HIP(hipMalloc((void**)&m->fde_nprm, 960 * 8 * sizeof(float)));
    for (int i = first; i < 5; ++i) {
        const int64_t wo = m->dir[mats[i][0]];
        SAPCU_TRY(launch_pack_frag_weights((const _Float16*)m->w16_hi + wo, (const _Float16*)m->w16_lo + wo, mats[i][1], mats[i][2],
                                           (_Float16*)m->fde_w + m->fde_off[i], nullptr));
    }
    static const int nslot[4] = {FD_SNN0, FD_SNN1, FD_SNN2, FD_SNN3};
    for (int i = 0; i < 4; ++i) SAPCU_TRY(launch_pack_fd_neuron(m->p(nslot[i]), FD_COUT[i], i < 2 ? 1 : 0, FD_COFF[i], m->fde_nprm, nullptr));
    SAPCU_CHECK_HIP(hipDeviceSynchronize());
    return SAPCU_OK;
}

int sapcu_model_create(int kind, const int32_t* hp, int n_hp, const float* blob, int64_t blob_floats,
                       const int64_t* dir_host, int n_dir, sapcu_model_t* out) {
    SAPCU_CHECK_ARG(hp && blob && dir_host && out && blob_floats > 0, "model_create: null pointer");
    // owns the handle until it is handed out: a failing stage frees whatever the stages before it allocated (free_model)
    std::unique_ptr<sapcu_model, void (*)(sapcu_model*)> owner(new (std::nothrow) sapcu_model(), free_model);
    sapcu_model* const m = owner.get();
    SAPCU_CHECK_ARG(m != nullptr, "model_create: out of host memory");
    m->kind = kind;
    read_env_switches(m);
    SAPCU_CHECK_ARG(kind == SAPCU_KIND_FN || kind == SAPCU_KIND_FD, "model_create: unknown kind %d", kind);
    SAPCU_TRY(kind == SAPCU_KIND_FN ? parse_fn_hparams(m, hp, n_hp, n_dir) : parse_fd_hparams(m, hp, n_hp, n_dir));
    SAPCU_TRY(check_slot_directory(m, dir_host, n_dir, blob_floats));
    SAPCU_TRY(copy_blob_and_fold(m, blob, blob_floats));
    SAPCU_TRY(split_blob_f16(m));
    SAPCU_TRY(pack_fn_chain_weights(m));
    SAPCU_TRY(pack_fd_encoder(m));
    *out = owner.release();
    return SAPCU_OK;
}

// Test hook, not part of include/sapcu.h (HOST pointers, no device work): the routine sapcu_model_create folds out_proj and fc2 of an
// fn block with — w_out [d, d], b_out [d], w_fc2 [n, d], b_fc2 [n] -> w_fold_out [n, d], b_fold_out [n].
int sapcu_internal_fold_affine_host(const float* w_out, const float* b_out, const float* w_fc2, const float* b_fc2, int d, int n,
                                    float* w_fold_out, float* b_fold_out) {
    SAPCU_CHECK_ARG(w_out && b_out && w_fc2 && b_fc2 && w_fold_out && b_fold_out && d >= 1 && n >= 1, "fold_affine: bad argument");
    fold_affine_f64(w_out, b_out, w_fc2, b_fc2, d, n, w_fold_out, b_fold_out);
    return SAPCU_OK;
}

int sapcu_model_destroy(sapcu_model_t m) {
    if (!m) return SAPCU_OK;
    free_model(m);
    return SAPCU_OK;
}

int64_t sapcu_workspace_bytes(sapcu_model_t m, int64_t b, int m_pts) {
    if (!m || b < 0 || m_pts < 1 || m_pts > 128) {
        set_error("workspace_bytes: bad argument");
        return SAPCU_ERR_ARG;
    }
    // the layout on a null base + the bytes the forward's align-up of the caller's pointer may cost
    const size_t bytes = m->kind == SAPCU_KIND_FN ? fn_ws_layout(nullptr, m, fn_plan(m, b, m_pts), m_pts).bytes
                                                  : fd_ws_layout(nullptr, m, fd_plan(m, b, m_pts), m_pts).bytes;
    return (int64_t)bytes + 256;
}

int sapcu_model_gate_violations(sapcu_model_t m, int* count_host) {
    SAPCU_CHECK_ARG(m && count_host, "gate_violations: null pointer");
    *count_host = 0;
    if (m->gate_dev) SAPCU_CHECK_HIP(hipMemcpy(count_host, m->gate_dev, sizeof(int), hipMemcpyDeviceToHost));
    return SAPCU_OK;
}

int sapcu_model_gemm_mode(sapcu_model_t m, int* split_f16_host, int* range_overflows_host) {
    SAPCU_CHECK_ARG(m && split_f16_host && range_overflows_host, "gemm_mode: null pointer");
    *split_f16_host = m->sf16 ? 1 : 0;
    *range_overflows_host = 0;
    if (m->ovf_dev) SAPCU_CHECK_HIP(hipMemcpy(range_overflows_host, m->ovf_dev, sizeof(int), hipMemcpyDeviceToHost));
    return SAPCU_OK;
}

int sapcu_model_fused_blocks(sapcu_model_t m, int m_pts, int* mask_host) {
    SAPCU_CHECK_ARG(m && mask_host && m_pts >= 1 && m_pts <= 128, "fused_blocks: bad argument");
    int mask = 0;
    if (m->kind == SAPCU_KIND_FN) {
        for (int l = 0; l < 3; ++l)
            if (fn_block_fused(m, l, m_pts)) mask |= 1 << l;
    } else {
        if (fd_encoder_fused(m, m_pts)) mask = 1;
        else if (fd_x0_path(m, m_pts)) mask = 2;
    }
    *mask_host = mask;
    return SAPCU_OK;
}

int sapcu_fn_forward(sapcu_model_t m, const float* patch, int64_t b, int m_pts, const int32_t* knn_in, int32_t* knn_out,
                     float* normals_out, void* workspace, int64_t ws_bytes, void* const* taps_host, void* stream) {
    SAPCU_CHECK_ARG(m && m->kind == SAPCU_KIND_FN, "fn_forward: not an fn model handle");
    SAPCU_CHECK_ARG(patch && normals_out && workspace, "fn_forward: null pointer");
    SAPCU_CHECK_ARG(b >= 0 && m_pts >= 1 && m_pts <= 128, "fn_forward: need 1 <= m_pts <= 128 (got %d)", m_pts);
    return fn_forward(m, patch, b, m_pts, knn_in, knn_out, normals_out, workspace, ws_bytes, taps_host,
                      (hipStream_t)stream);
}

int sapcu_fd_forward(sapcu_model_t m, const float* patch, int64_t b, int m_pts, const int32_t* knn_force, float* dist_out,
                     void* workspace, int64_t ws_bytes, void* const* taps_host, void* stream) {
    SAPCU_CHECK_ARG(m && m->kind == SAPCU_KIND_FD, "fd_forward: not an fd model handle");
    SAPCU_CHECK_ARG(patch && dist_out && workspace, "fd_forward: null pointer");
    SAPCU_CHECK_ARG(b >= 0 && m_pts >= 1 && m_pts <= 128, "fd_forward: need 1 <= m_pts <= 128 (got %d)", m_pts);
    return fd_forward(m, patch, b, m_pts, knn_force, dist_out, workspace, ws_bytes, taps_host, (hipStream_t)stream);
}

}  // extern "C"
