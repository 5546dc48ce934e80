// kernels_scene.hip -- how much the picture changed between two RGB8 frames: the block-histogram distance behind fav_stylize -scene_cut.
//
//   luma    Y = (77 R + 150 G + 29 B + 128) >> 8 (0..255);  bin = Y >> 3 (32 bins)
//   grid    4 x 4 cells; cell (cx, cy) covers x in [cx W/4, (cx+1) W/4), y in [cy H/4, (cy+1) H/4), floor division (W, H >= 4)
//   cell    d[cy*4+cx] = sum over bins |hist_prev[cell][bin] - hist_cur[cell][bin]|;  total = sum over cells  (uint32: <= 2 W H <= 2^29)
// Integer arithmetic throughout, and integer adds commute: the 17 numbers depend on the two frames and on nothing else (no schedule, no
// grid size), and tests/util/scene_model.py restates them in numpy: the kernels are held to that model for equality.
//
// Shape.  Three operations on the caller's queue:
//   1. the 2 KB workspace -- the SIGNED difference table [16 cells][32 bins], +1 per pixel of `prev`, -1 per pixel of `cur` -- is zeroed
//      (one memset of the whole block, which starts the allocation and is a multiple of 16 bytes);
//   2. scene_hist_kernel, one pass over both frames.  The frames are walked as ONE run of W*H pixels (rows are 3 W bytes and follow each
//      other without padding), a lane takes 16 consecutive pixels = 48 bytes of each frame per step: one 48-byte access per frame,
//      declared unaligned like the planes of kernels_yuv.hip (neither the base nor a row is aligned; for an aligned base they are three
//      16-byte loads).  Only the last chunk of the frame can be short; it goes byte by byte.  Nothing outside [base, base + 3 W H) is read.
//      A lane follows (x, y) of its pixels incrementally, so a chunk may cross rows and cells.
//      Histogram update: a table PER WAVE in LDS (4 x 2 KB), and a lane adds RUNS -- equal (cell, bin) of consecutive pixels are counted
//      in a register and reach LDS as one add.  A constant frame (black frames around a cut) would otherwise send 64 lanes x 16 pixels to
//      one LDS word; with runs it is one add per lane and chunk, and when the whole wave ends a chunk on the same word (constant and
//      smooth frames) the wave sums its counts with shuffles and ONE lane adds.  The block then sums its four tables and adds the
//      non-zero entries to the workspace with device-scope integer atomics (a block covers a few rows: most of its 512 entries are zero).
//   3. scene_finish_kernel, one block: |.|, the 16 cell sums, the total, into `result` (device or host-mapped memory; a system-scope
//      fence follows the stores, as behind the size word of the PNG encoder).
// The sums are formed by a second launch, not by the last block of the first to finish: between kernels of one queue the table is visible
// without any protocol, while a ticket needs a release / acquire pair per block whose pitfalls on this hardware outnumber the launch it
// saves (about 5 us of the 15 us a call takes back to back, DESIGN.md "Scene changes") -- on a queue that is not the frame's.
#include "fav_internal.h"

namespace fav {

namespace {

constexpr int SC_NT = 256;                 // 4 waves
constexpr int SC_WAVES = SC_NT / 64;
constexpr int SC_PX = 16;                  // pixels of a lane's chunk
constexpr int SC_TABLE = 16 * 32;          // (cell, bin)
constexpr int SC_MAX_BLOCKS = 1024;

struct __attribute__((packed, aligned(1))) B48 { uint32_t v[12]; };

__device__ __forceinline__ uint32_t byte_at(const uint32_t* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// a lane's run of equal keys: (key, count) in registers, flushed into the wave's table when the key changes
struct Run {
    int key, cnt;
    __device__ __forceinline__ void add(int k, int* hist, int sign)
    {
        if (k == key) { ++cnt; return; }
        if (cnt) atomicAdd(hist + key, sign * cnt);
        key = k; cnt = 1;
    }
};

// the end of a chunk: the lanes' open runs.  All 64 lanes on one word (constant frames, smooth ones): summed in the wave, one add.
__device__ __forceinline__ void flush_run(const Run& r, int* hist, int sign, int lane)
{
    const int first = __builtin_amdgcn_readfirstlane(r.key);
    if (__all(r.key == first)) {           // (wave-uniform branch; lanes without pixels hold key -1: a wave with such lanes and others is not uniform)
        int c = r.cnt;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0 && first >= 0 && c) atomicAdd(hist + first, sign * c);
    } else if (r.cnt) atomicAdd(hist + r.key, sign * r.cnt);
}

__global__ __launch_bounds__(SC_NT) void scene_hist_kernel(const uint8_t* prev, const uint8_t* cur, int W, int H, int* table)
{
    __shared__ int hist[SC_WAVES][SC_TABLE];
    const int t = threadIdx.x, lane = t & 63;
    int* const mine = hist[t >> 6];
    for (int i = t; i < SC_WAVES * SC_TABLE; i += SC_NT) (&hist[0][0])[i] = 0;
    __syncthreads();

    const unsigned npx = (unsigned)W * (unsigned)H;                       // <= 2^28 (launch_scene_change)
    const unsigned nchunks = (npx + SC_PX - 1) / SC_PX;
    const int bx1 = W / 4, bx2 = 2 * W / 4, bx3 = 3 * W / 4, by1 = H / 4, by2 = 2 * H / 4, by3 = 3 * H / 4;
    // the trip count is the block's, not the lane's: every lane of a wave reaches the shuffles of flush_run
    for (unsigned c0 = blockIdx.x * SC_NT; c0 < nchunks; c0 += gridDim.x * SC_NT) {
        const unsigned c = c0 + t;
        const unsigned p0 = c * SC_PX;
        const int n = c < nchunks ? (int)min((unsigned)SC_PX, npx - p0) : 0;
        uint32_t a[12], b[12];
        if (n == SC_PX) {
            const B48 va = *reinterpret_cast<const B48*>(prev + 3 * (size_t)p0), vb = *reinterpret_cast<const B48*>(cur + 3 * (size_t)p0);
#pragma unroll
            for (int i = 0; i < 12; ++i) { a[i] = va.v[i]; b[i] = vb.v[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) a[i] = b[i] = 0u;
#pragma unroll
            for (int i = 0; i < 3 * SC_PX; ++i)                               // the frame's last pixels: byte by byte, inside the frame
                if (i < 3 * n) {
                    a[i >> 2] |= (uint32_t)prev[3 * (size_t)p0 + i] << (8 * (i & 3));
                    b[i >> 2] |= (uint32_t)cur[3 * (size_t)p0 + i] << (8 * (i & 3));
                }
        }
        int y = (int)(p0 / (unsigned)W), x = (int)(p0 - (unsigned)y * (unsigned)W);
        int rowcell = 4 * ((y >= by1) + (y >= by2) + (y >= by3));
        Run rp{-1, 0}, rc{-1, 0};
#pragma unroll
        for (int i = 0; i < SC_PX; ++i) {
            if (i < n) {
                const int cell = rowcell + (x >= bx1) + (x >= bx2) + (x >= bx3);
                const uint32_t ya = 77u * byte_at(a, 3 * i) + 150u * byte_at(a, 3 * i + 1) + 29u * byte_at(a, 3 * i + 2) + 128u;
                const uint32_t yb = 77u * byte_at(b, 3 * i) + 150u * byte_at(b, 3 * i + 1) + 29u * byte_at(b, 3 * i + 2) + 128u;
                rp.add(cell * 32 + (int)(ya >> 11), mine, 1);                // (Y >> 3 = (.. + 128) >> 8 >> 3)
                rc.add(cell * 32 + (int)(yb >> 11), mine, -1);
                if (++x == W) { x = 0; ++y; rowcell = 4 * ((y >= by1) + (y >= by2) + (y >= by3)); }
            }
        }
        flush_run(rp, mine, 1, lane);
        flush_run(rc, mine, -1, lane);
    }
    __syncthreads();
    for (int i = t; i < SC_TABLE; i += SC_NT) {
        int v = 0;
#pragma unroll
        for (int w = 0; w < SC_WAVES; ++w) v += hist[w][i];
        if (v) __hip_atomic_fetch_add(table + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one block of 512: thread = (cell, bin)
__global__ __launch_bounds__(SC_TABLE) void scene_finish_kernel(const int* table, fav_scene_change* result)
{
    __shared__ uint32_t d[16];
    const int t = threadIdx.x;
    const int v = table[t];
    uint32_t s = (uint32_t)(v < 0 ? -v : v);
#pragma unroll
    for (int k = 16; k > 0; k >>= 1) s += __shfl_xor(s, k);                   // the 32 bins of a cell are half a wave
    if ((t & 31) == 0) d[t >> 5] = s;
    __syncthreads();
    // `result` may be host-mapped.  `total` is stored LAST, behind system-scope fences: a host that set it to a value no total can take
    // (> 2^29) and polls it finds the cells complete -- the way the PNG encoder's size word is used
    if (t < 16) { result->cell[t] = d[t]; __threadfence_system(); }
    __syncthreads();
    if (t == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) total += d[k];
        result->total = total;
        __threadfence_system();
    }
}

}  // namespace

size_t scene_change_workspace_bytes() { return SC_TABLE * sizeof(int); }

int launch_scene_change(const uint8_t* prev, const uint8_t* cur, int W, int H, void* workspace, fav_scene_change* result, hipStream_t st)
{
    int* const table = static_cast<int*>(workspace);
    FAV_HIP(hipMemsetAsync(table, 0, scene_change_workspace_bytes(), st));
    const unsigned nchunks = ((unsigned)W * (unsigned)H + SC_PX - 1) / SC_PX;
    const unsigned need = (nchunks + SC_NT - 1) / SC_NT, blocks = need < SC_MAX_BLOCKS ? need : SC_MAX_BLOCKS;
    hipLaunchKernelGGL(scene_hist_kernel, dim3(blocks), dim3(SC_NT), 0, st, prev, cur, W, H, table);
    FAV_LAUNCH_CHECK("scene_hist_kernel");
    hipLaunchKernelGGL(scene_finish_kernel, dim3(1), dim3(SC_TABLE), 0, st, (const int*)table, result);
    FAV_LAUNCH_CHECK("scene_finish_kernel");
    return FAV_OK;
}

}  // namespace fav
