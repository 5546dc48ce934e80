// Private to the host side of the transformer network: net_model.cpp (a checkpoint's layers -> their device form), net.cpp (kernel
// selection, the executor, fav_net's C ABI) and ops.cpp (the stand-alone operators).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "dev_owned.h"

namespace fav {

struct DevBuf { void* p = nullptr; size_t bytes = 0; };
struct DevConvW {
    float* wgt = nullptr; float* bias = nullptr; unsigned short* wgt16 = nullptr;      // repack_weights() form: the generic, c8 and halo-resident kernels
    float* packed[CONV_KERNELS] = {};      // by ConvKernel: the form that kernel's own packing gives (upload_layers); null: that kernel cannot be selected
    ConvShape s;                           // the layer, nothing pending on its input (select_conv asks with the state the input is then in)
    int kpad = 0;
};
struct DevIN { float* gamma = nullptr; float* beta = nullptr; float* scale = nullptr; float* shift = nullptr;
               long long* acc = nullptr; size_t acc_bytes = 0; };      // accumulator form of the statistics (fav_internal.h, Affine::acc1): [2 parities][stat_acc_words(C)], zero between frames

struct Act {
    float* data = nullptr;
    int Hp = 0, Wp = 0;          // physical size
    int C = 0;                   // channel pitch
    int ups = 0;                 // pending nearest upsample (log2)
    Affine pre;                  // pending per-channel transform
    float* partials = nullptr;   // (mean, M2) tiles of the raw tensor from the producing conv, or null
    int mblocks = 0, ppitch = 0;
    int* counts = nullptr;       // per-partial pixel counts (first-layer kernel) or null
    int pitch = 0;               // row pitch in pixels when the tensor sits inside a wider allocation (0: Wp)
    // pending residual join (conv3_wino_kernel MODE 2): data = the branch's raw output, pre = its InstanceNorm, join_skip = the skip
    // tensor's pixel under data's pixel (0, 0) at the same pitch; join_out = where the consuming convolution writes the joined tensor
    const float* join_skip = nullptr; float* join_out = nullptr;
    long long* acc = nullptr; long long* acc_other = nullptr;      // the producing convolution added its statistics to accumulators (this frame's parity | the other one)
    int H() const { return Hp << ups; }
    int W() const { return Wp << ups; }
    int P() const { return pitch ? pitch : Wp; }
};

// The input state a kernel is built for, as the (stages, ups) of a ConvShape: packing asks with it whether the kernel can EVER run the
// layer; select_conv() asks again per forward, with the state the input is then in
struct InputState { int stages, ups; };
constexpr InputState IN_PLAIN{0, 0};        // nothing pending: the network input (first layer); also asked for the residual 3x3 convolutions, which take 0 or 1 norms
constexpr InputState IN_NORM{1, 0};         // one pending norm (+ ReLU), no upsampling: the stride-2 layers
constexpr InputState IN_NORM_UP2{1, 1};     // one pending norm behind a x2 upsampling: up2
inline ConvShape with_input(ConvShape s, InputState in) { s.stages = in.stages; s.ups = in.ups; return s; }

// Everything fav_net knows about one ConvKernel: conv_kernel(k), row k of CONV_KERNEL_TABLE (net_model.cpp).  N = the padded output channel
// count COUTp; the profile ids are a contract (fav_internal.h, enum ConvKernel)
enum ProfileId { ID_FIXED, ID_PLUS_N, ID_PLUS_N_JOIN, ID_N_TILE };      // id | id + N | id + N (+ 1: a pending residual join as the input) | the generic kernel's N tile: 32 | 64 | 128
struct ConvKernelInfo {
    ConvKernel kernel;
    const char* name;
    const char* off_switch;                                                  // FAV_NO_<kernel> (diagnostic build): select_conv() passes the kernel over; null: none
    bool (*eligible)(const ConvShape&);                                      // null: takes every layer
    InputState pack_state;
    void (*pack)(const float* w, const ConvShape&, std::vector<float>&);     // the kernel's own form of the weights; null: it reads wgt / wgt16
    int (*tiles)(const ConvLaunch&);                                         // partial-statistics tiles of an OH x OW output; null: none (the last layer)
    bool counts;                                                             // writes the tiles' pixel counts (else every tile but the last holds CONV_BM pixels)
    int id; ProfileId id_rule;
    int (*launch)(const ConvLaunch&, hipStream_t);
    bool hands_over;      // its blocks hand tiles over to each other: launched with no_sk set while look-ahead masks are in flight (timed_conv)
};
const ConvKernelInfo& conv_kernel(ConvKernel k);

// Tuning / ablation switches (not part of the product contract): read ONCE per process, never on the launch path.
struct Tuning {
    bool off[CONV_KERNELS];                                           // ConvKernelInfo::off_switch is set
    bool first_1d = diag_env("FAV_FIRST_1D") != nullptr;              // the 1-D form of the first layer
    bool wino_f2 = diag_env("FAV_WINO_F2") != nullptr;                // the residual convolutions as F(2x2,3x3) (rounds 2-3) instead of F(4x4,3x3)
    bool no_acc_stats = diag_env("FAV_NO_ACC_STATS") != nullptr;      // every InstanceNorm through partials + an in_finalize launch (rounds 1-4)
    bool no_lazy_join = diag_env("FAV_NO_LAZY_JOIN") != nullptr;      // no residual join stays pending | with the F(4x4) kernels too (run(), L_RES)
    bool lazy_join = diag_env("FAV_LAZY_JOIN") != nullptr;
    int side_sk = diag_env("FAV_SIDE_SK") ? atoi(diag_env("FAV_SIDE_SK")) : 0;      // 1: stream-K stays next to the side queues, 2: for the stride-2 halo kernel only
    Tuning() { for (int k = 0; k < CONV_KERNELS; ++k) { const char* sw = conv_kernel((ConvKernel)k).off_switch; off[k] = sw && diag_env(sw); } }
};
const Tuning& tuning();

// net_model.cpp
void repack_weights(const Layer& L, int cinp, int coutp, int kpad, std::vector<float>& out);
bool only_tail(const std::vector<Layer>& ls, size_t from, bool& has_tanh, float& mul);      // nothing but Tanh / MulConstant / Identity from ls[from] on

}  // namespace fav

struct fav_net {
    int device = 0;
    std::vector<fav::Layer> layers;    // as parsed from the checkpoint (describe / output size / parameter count)
    std::vector<fav::Layer> exec;      // what runs: the same network with channel counts padded to powers of two (pad_channel_counts); Layer::dev_index -> convs / ins
    int pad = 0;                  // leading nn.SpatialReflectionPadding (train_video.lua:319-325)
    bool pad_folded = false;      // ... folded into the input assembly (layers[0] is then skipped by the executor)
    int in_channels = 0;
    long long params = 0;
    std::vector<fav::DevConvW> convs;  // traversal order
    std::vector<fav::DevIN> ins;
    // Device memory that lives as long as the net has ONE owner list: dev_new / dev_put (net_model.cpp) allocate, append the allocation to
    // `owned` and hand out a raw view.  convs, ins and the scalars below keep those views, so the launch records read plain pointers
    std::vector<fav::dev_ptr<void>> owned;
    template <class T> int dev_new(T** view, size_t n, bool zeroed = false);
    template <class T> int dev_put(T** view, const std::vector<T>& h, size_t pad_to = 0);
    float* ones = nullptr; float* zeros = nullptr;
    float* sk_ws = nullptr; unsigned* sk_flags = nullptr; unsigned sk_epoch = 0;   // stream-K hand-off state
    float* ks_ws = nullptr; int* ks_cnt = nullptr;                                    // meeting places of the F(4x4) Winograd kernel's stream-K launches
    // a residual block whose join stays pending (run(), L_RES): its last convolution lays its output out under the skip tensor
    struct LazyOut { bool active = false; int pitch = 0, rows = 0, shave = 0, conv_index = -1; } lazy;
    fav::host_ptr<unsigned> sk_err_host; unsigned* sk_err_dev = nullptr;           // host-mapped: a hand-off wait timed out (sk_err_dev: its device address)
    bool shared_device = false;     // data-parallel grids only: set by the caller (fav_net_set_shared_device) or by a timed-out hand-off
    int precision = 0;              // 0 = fp32 (parity mode), 1 = bf16 operands in the halo-resident 3x3 convolutions (fast mode)
    int acc_parity = 0;             // which half of the InstanceNorm accumulators this forward adds to (the consumers zero the other half)
    bool acc_dirty = false;         // a forward failed half-way (or the precision changed): every accumulator is zeroed before the next forward
    bool branch_tail_acc_ok = false; // set by L_RES around its branch: the join is a plain res_add launch, which takes the last InstanceNorm as accumulators
    int reserve_cus = 0;            // set when a stream uses the look-ahead side queues (they are CU-masked to this many CUs)
    // activation arena: buffers are created on the first forward for a given (H, W) and reused after
    int curH = 0, curW = 0;
    std::vector<fav::DevBuf> bufs;
    // ... carved out of a few large slabs: sixty hipMalloc calls cost the first frame of a run 10 ms (profiles/e2e_r04s_startup.log)
    std::vector<fav::dev_ptr<void>> slabs; char* slab_cur = nullptr; size_t slab_left = 0;
    size_t cursor = 0;
    hipStream_t st = nullptr;
    fav::dev_ptr<float> stage; size_t stage_bytes = 0;   // NCHW-boundary staging (fav_net_forward)
    // optional per-convolution event timing (bench.py roofline)
    bool profiling = false;
    struct ProfRec { fav::event_h a, b; int conv; };
    std::vector<ProfRec> prof_pending;
    std::vector<double> prof_ms, prof_macs; std::vector<int> prof_n, prof_tile;

    ~fav_net() { (void)hipSetDevice(device); }      // (the members free themselves, on the net's device)
    // net_model.cpp
    int upload_layers(std::vector<fav::Layer>& ls, int& chan_pitch, int& maxc);
    int upload();
    // net.cpp
    int alloc(size_t bytes, float** out);
    int timed_conv(const fav::ConvLaunch& c, const fav::Layer& L, fav::ConvKernel kernel);
    int run(std::vector<fav::Layer>& ls, fav::Act& cur, bool top, float* out_planar, float* out_raw);
    bool res_block_is_winograd(const fav::Layer& R) const;
    bool acc_stats_ok(const std::vector<fav::Layer>& ls, size_t li) const;
    int forward_padded(const float* in8, int H, int W, float* out_planar, float* out_raw, hipStream_t stream);
    int forward_padded_unordered(const float* in8, int H, int W, float* out_planar, float* out_raw, hipStream_t stream);
    void out_size(int H, int W, int* Ho, int* Wo) const;
};
