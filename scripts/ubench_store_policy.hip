// scripts/ubench_store_policy.hip -- how should integrate_free's state stores leave the chip?  A compute-free kernel with the lean
// launch's access pattern on the slab of dmx_internal.hpp (tiles of 64 bodies, 30 components): components 1, 3-6, 8, 10-12 loaded,
// 1, 3-6, 8 stored back in place with a changed value (pattern "lean"); or step_plane's moves, 0-12 loaded and 0-12 stored
// (pattern "13/13").  256-thread workgroups, a grid that is a multiple of 8, the tile sweep of dmx_sweep.hpp alternating from one
// launch to the next.  The stores take one of four forms:
//   plain   So[ix] = v                                                          global_store_dword
//   wt      __hip_atomic_store(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)   global_store_dword ... sc1   (write-through)
//   nt      __builtin_nontemporal_store(v, p)                                   global_store_dword ... nt
//   wt+nt   __builtin_amdgcn_raw_buffer_store_b32/b64(bits, tile's resource, offset, 0, sc1 | nt)   buffer_store_dword ... sc1 nt
// Every form is a vector store.  Each cell is 300 launches back to back on one stream after 40 warm-up launches, timed by
// events, five times over with the cells interleaved (median and spread = max - min are reported).  Beside each cell its control:
// the reverse direction is the plain G8 - 1 - b, which sends a tile group to the XCD of 7 - b%8 (profiles/ab_sweep.txt's control), so
// sweep - control is the L2 reuse from one launch to the next that survives the store form.
// Build: hipcc --offload-arch=gfx950 -O3 -I rl-ode-physics_amd/csrc -o ubench_store_policy scripts/ubench_store_policy.hip
// Run:   ./ubench_store_policy            (slab contents pseudo-random: zero lines move faster, profiles/r03_ubench_fill_effect.txt)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdint.h>
#include "dmx_sweep.hpp"
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int TILE = 64, NCOMP = 30;        // SLAB_TILE, C_COUNT
enum : int { PLAIN = 0, WT = 1, NT = 2, WTNT = 3, NFORM = 4 };
enum : int { LEAN = 0, ALL13 = 1 };
static const char *form_name[NFORM] = { "plain", "wt (sc1)", "nt", "wt+nt (sc1 nt)" };

template <class T> struct Bits;
template <> struct Bits<float> { using type = uint32_t; };
template <> struct Bits<double> { using type = uint64_t; };

// component k of the tile `tile` (wave-uniform), lane j: the four store forms
template <int FORM, class T> __device__ __forceinline__ void store_form(T *S, int64_t tile, int k, int j, T v)
{
    using U = typename Bits<T>::type;
    T *p = S + tile * (NCOMP * TILE) + k * TILE + j;
    if constexpr (FORM == PLAIN) *p = v;
    else if constexpr (FORM == WT) __hip_atomic_store((U *)p, __builtin_bit_cast(U, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if constexpr (FORM == NT) __builtin_nontemporal_store(v, p);
    else {
        // the tile as a buffer of its own: the offset stays below 2^32 at any slab size, and the hardware refuses an offset beyond the tile
        __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(S + tile * (NCOMP * TILE), 0, NCOMP * TILE * (int)sizeof(T), 0x00020000);
        constexpr int aux = 16 | 2;     // sc1 | nt
        if constexpr (sizeof(T) == 4) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, (k * TILE + j) * 4, 0, aux);
        else {
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (k * TILE + j) * 8, 0, aux);
        }
    }
}

// CTL = 0: dmx::sweep_block; 1: the control, whose reverse direction moves a tile group to another XCD
template <class T, int FORM, int PAT, int CTL> __global__ __launch_bounds__(256) void k_pass(T *S, int64_t n, int rev)
{
    using U = typename Bits<T>::type;
    const unsigned b = CTL ? (rev ? gridDim.x - 1 - blockIdx.x : blockIdx.x) : dmx::sweep_block(blockIdx.x, gridDim.x, rev);
    const int64_t i = b * (int64_t)256 + threadIdx.x;
    if (i >= n) return;         // n is a multiple of 256 here; the slab is allocated for all of [0, n)
    const int64_t tile = __builtin_amdgcn_readfirstlane((int)(i >> 6));
    const int j = threadIdx.x & 63;
    const T *p = S + tile * (NCOMP * TILE) + j;
    T c[13];
#pragma unroll
    for (int k = 0; k < 13; k++) {
        const bool lean_load = k == 1 || (k >= 3 && k <= 6) || k == 8 || k >= 10;
        c[k] = (PAT == ALL13 || lean_load) ? p[k * TILE] : T(0);
    }
    // the changed value: bit 0 of the mantissa flips, bit 1 follows the components that are only read (keeps their loads alive)
    const U m = U(1) | ((__builtin_bit_cast(U, c[10]) ^ __builtin_bit_cast(U, c[11]) ^ __builtin_bit_cast(U, c[12])) & U(2));
#pragma unroll
    for (int k = 0; k < 13; k++) {
        const bool lean_store = k == 1 || (k >= 3 && k <= 6) || k == 8;
        if (PAT == ALL13 || lean_store) store_form<FORM>(S, tile, k, j, __builtin_bit_cast(T, (U)(__builtin_bit_cast(U, c[k]) ^ m)));
    }
}

template <class T> __global__ void k_fill(T *a, size_t n)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned h = (unsigned)i * 2654435761u; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    a[i] = T(0.5) + T(h & 0xffffff) * T(1.0 / 16777216.0);
}

template <class T, int FORM, int PAT, int CTL> static double cell_us(T *S, int64_t n, int &rev)
{
    const unsigned grid = dmx::sweep_grid((unsigned)((n + 255) / 256));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 40; i++) k_pass<T, FORM, PAT, CTL><<<grid, 256>>>(S, n, rev++ & 1);
    CHECK(hipEventRecord(e0, 0));
    for (int i = 0; i < 300; i++) k_pass<T, FORM, PAT, CTL><<<grid, 256>>>(S, n, rev++ & 1);
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipGetLastError());
    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
    CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
    return ms * 1e3 / 300;
}

template <class T, int PAT, int FORM> static void form_cells(T *S, int64_t n, int &rev, int r, double (*t)[2][5])
{
    t[FORM][0][r] = cell_us<T, FORM, PAT, 0>(S, n, rev);
    t[FORM][1][r] = cell_us<T, FORM, PAT, 1>(S, n, rev);
}

template <class T, int PAT> static void shape(int64_t n)
{
    T *S;
    const size_t elems = (size_t)n * NCOMP;
    CHECK(hipMalloc(&S, elems * sizeof(T)));
    k_fill<T><<<(unsigned)((elems + 255) / 256), 256>>>(S, elems);
    CHECK(hipDeviceSynchronize());
    double t[NFORM][2][5];
    int rev = 0;
    for (int r = 0; r < 5; r++) {       // the cells interleaved: a drift of the machine falls on all of them alike
        form_cells<T, PAT, PLAIN>(S, n, rev, r, t);
        form_cells<T, PAT, WT>(S, n, rev, r, t);
        form_cells<T, PAT, NT>(S, n, rev, r, t);
        form_cells<T, PAT, WTNT>(S, n, rev, r, t);
    }
    const int nin = PAT == LEAN ? 9 : 13, nout = PAT == LEAN ? 6 : 13;
    printf("## %s, %lld bodies, pattern %s: %d reals in, %d out per body = %.1f MB read, %.1f MB written per launch\n",
           sizeof(T) == 4 ? "f32" : "f64", (long long)n, PAT == LEAN ? "lean" : "13/13", nin, nout,
           n * (double)nin * sizeof(T) / 1e6, n * (double)nout * sizeof(T) / 1e6);
    for (int f = 0; f < NFORM; f++) {
        double med[2], spr[2];
        for (int c = 0; c < 2; c++) {
            std::sort(t[f][c], t[f][c] + 5);
            med[c] = t[f][c][2]; spr[c] = t[f][c][4] - t[f][c][0];
        }
        printf("CELL %-3s %9lld %-5s %-15s sweep median %9.3f us spread %6.3f   control median %9.3f us spread %6.3f   control - sweep %+8.3f\n",
               sizeof(T) == 4 ? "f32" : "f64", (long long)n, PAT == LEAN ? "lean" : "13/13", form_name[f], med[0], spr[0], med[1], spr[1],
               med[1] - med[0]);
    }
    fflush(stdout);
    CHECK(hipFree(S));
}

int main()
{
    printf("# store forms of the in-place state write-back: us per launch, 300 launches back to back after 40, five repeats per cell\n");
    shape<float, LEAN>(1 << 20);
    shape<double, LEAN>(1 << 20);
    shape<float, LEAN>(1 << 24);
    shape<double, LEAN>(1 << 24);
    shape<float, ALL13>(1 << 18);
    shape<double, ALL13>(1 << 18);
    return 0;
}
