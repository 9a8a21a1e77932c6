// cross_scan.hip -- CrossScan / CrossMerge (4-route 2-D unrolling) and the two-view channel swap.
//
// Semantics: models/csm_triton.py:22-85 (cross_scan_fwd / cross_merge_fwd, scans=0, channel-first)
// and models/fusion_vmamba.py:189-213 (SwappingScan_multiview.forward).  Pure data movement, so
// the design goal is that every HBM access has lanes along the contiguous axis: a workgroup
// stages a run of whole (b, c) planes in LDS (coalesced), and the column-major routes are read
// out of LDS with an odd row pitch instead of being gathered from HBM with a stride.
#include "xfm_common.hpp"

namespace xfm {

// LDS pitch for an H x W plane so that walking a column (stride = pitch) is bank-conflict free.
__host__ __device__ inline int odd_pitch(int w) { return w | 1; }

// x: (P, H, W) planes -> y: per batch (4, C, L).  One workgroup handles `pp` consecutive planes.
template <typename T>
__global__ void __launch_bounds__(256) cross_scan_kernel(const T *__restrict__ x, T *__restrict__ y, int planes, int C,
                                                         int H, int W, int pp) {
    extern __shared__ float smem[];
    const int L = H * W, pitch = odd_pitch(W), psz = H * pitch;
    const int p0 = blockIdx.x * pp;
    const int np = min(pp, planes - p0);
    const int total = np * L;
    // coalesced load of np contiguous planes into the padded LDS layout
    for (int e = threadIdx.x; e < total; e += 256) {
        const int pl = e / L, l = e - pl * L;
        const int h = l / W, w = l - h * W;
        smem[pl * psz + h * pitch + w] = ldf<T>(x + (int64_t)p0 * L + e);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += 256) {
        const int pl = e / L, l = e - pl * L;
        const int plane = p0 + pl;
        const int b = plane / C, c = plane - b * C;
        T *yb = y + ((int64_t)b * 4 * C + c) * L;  // route k adds k*C*L
        const int64_t ks = (int64_t)C * L;
        // row-major value at l, and column-major value at l (= x[l % H][l / H])
        const int h0 = l / W, w0 = l - h0 * W;
        const float vr = smem[pl * psz + h0 * pitch + w0];
        const int w1 = l / H, h1 = l - w1 * H;
        const float vc = smem[pl * psz + h1 * pitch + w1];
        stf<T>(yb + l, vr);
        stf<T>(yb + ks + l, vc);
        stf<T>(yb + 2 * ks + (L - 1 - l), vr);
        stf<T>(yb + 3 * ks + (L - 1 - l), vc);
    }
}

// y: (B, 4, C, L) -> x: (B, C, L);  x[h*W+w] = y0[l] + y2[L-1-l] + y1[m] + y3[L-1-m], m = w*H+h.
template <typename Tin, typename Tout>
__global__ void __launch_bounds__(256) cross_merge_kernel(const Tin *__restrict__ y, Tout *__restrict__ x, int planes,
                                                          int C, int H, int W, int pp) {
    extern __shared__ float smem[];
    const int L = H * W, pitch = odd_pitch(H), psz = W * pitch;  // column-major planes: W rows of H
    const int p0 = blockIdx.x * pp;
    const int np = min(pp, planes - p0);
    const int total = np * L;
    const int64_t ks = (int64_t)C * L;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int pl = e / L, m = e - pl * L;
        const int plane = p0 + pl;
        const int b = plane / C, c = plane - b * C;
        const Tin *yb = y + ((int64_t)b * 4 * C + c) * L;
        const float v = ldf<Tin>(yb + ks + m) + ldf<Tin>(yb + 3 * ks + (L - 1 - m));
        const int w = m / H, h = m - w * H;
        smem[pl * psz + w * pitch + h] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += 256) {
        const int pl = e / L, l = e - pl * L;
        const int plane = p0 + pl;
        const int b = plane / C, c = plane - b * C;
        const Tin *yb = y + ((int64_t)b * 4 * C + c) * L;
        const int h = l / W, w = l - h * W;
        const float v = ldf<Tin>(yb + l) + ldf<Tin>(yb + 2 * ks + (L - 1 - l)) + smem[pl * psz + w * pitch + h];
        stf<Tout>(x + (int64_t)plane * L + l, v);
    }
}

// out[b,0,c,:] = (c even ? x2 : x)[b,c,:],  out[b,1,c,:] = (c even ? x : x2)[b,c,:]
template <typename T>
__global__ void __launch_bounds__(256) swap_scan_kernel(const T *__restrict__ x, const T *__restrict__ x2,
                                                        T *__restrict__ out, int64_t total, int C, int L) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / L;  // b*C + c
        const int l = (int)(e - row * L);
        const int64_t b = row / C;
        const int c = (int)(row - b * C);
        const bool even = (c & 1) == 0;
        const T a = x[e], bb = x2[e];
        T *o = out + ((b * 2) * C + c) * (int64_t)L + l;
        o[0] = even ? bb : a;
        o[(int64_t)C * L] = even ? a : bb;
    }
}

static int planes_per_block(int L, int pitch_plane_floats, int planes) {
    // aim for >= 2048 elements per workgroup, stay under 48 KiB of LDS, keep the grid >= 1024 blocks when possible
    int pp = (2048 + L - 1) / L;
    if (pp < 1) pp = 1;
    while (pp > 1 && (size_t)pp * pitch_plane_floats * sizeof(float) > 48 * 1024) --pp;
    while (pp > 1 && (planes + pp - 1) / pp < 1024) --pp;
    return pp;
}

template <typename T>
static int launch_scan(const void *x, void *y, int B, int C, int H, int W, hipStream_t s) {
    const int planes = B * C;
    const int psz = H * odd_pitch(W);
    const int pp = planes_per_block(H * W, psz, planes);
    const size_t lds = (size_t)pp * psz * sizeof(float);
    if (lds > 160 * 1024) return XFM_ELIMIT;
    hipLaunchKernelGGL((cross_scan_kernel<T>), dim3((planes + pp - 1) / pp), dim3(256), lds, s, (const T *)x, (T *)y,
                       planes, C, H, W, pp);
    return check_launch();
}

template <typename Tin, typename Tout>
static int launch_merge(const void *y, void *x, int B, int C, int H, int W, hipStream_t s) {
    const int planes = B * C;
    const int psz = W * odd_pitch(H);
    const int pp = planes_per_block(H * W, psz, planes);
    const size_t lds = (size_t)pp * psz * sizeof(float);
    if (lds > 160 * 1024) return XFM_ELIMIT;
    hipLaunchKernelGGL((cross_merge_kernel<Tin, Tout>), dim3((planes + pp - 1) / pp), dim3(256), lds, s,
                       (const Tin *)y, (Tout *)x, planes, C, H, W, pp);
    return check_launch();
}

// ---- route split / merge of the x_proj output ------------------------------------------------------------------
// x_proj is evaluated once on the map in natural order (the projection commutes with the route permutations); this
// kernel hands its (B, 4, R+2N, H*W) result to the consumers in the layout contract of xfm_ss2d_fwd: three contiguous
// tensors dt-input (B,4,R,L), Bs (B,4,N,L), Cs (B,4,N,L), with the planes of the column routes (k odd) transposed to
// column-major.  One workgroup per (b, k, c) plane; transposition through a padded LDS tile.
template <typename Ts, typename Td>
__device__ __forceinline__ void plane_move(const Ts *src, Td *dst, int R0, int C0, bool transpose, float *tile) {
    const int L = R0 * C0;
    if (!transpose) {
        for (int e = threadIdx.x; e < L; e += blockDim.x) stf<Td>(dst + e, ldf<Ts>(src + e));
        return;
    }
    const int pitch = C0 + 1;
    for (int e = threadIdx.x; e < L; e += blockDim.x) {
        const int r = e / C0, c = e - r * C0;
        tile[r * pitch + c] = ldf<Ts>(src + e);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < L; e += blockDim.x) {     // (R0 x C0) row-major -> (C0 x R0) row-major
        const int c = e / R0, r = e - c * R0;
        stf<Td>(dst + e, tile[r * pitch + c]);
    }
}

// Bs32 / Cs32 (optional): the same B / C rows once more as fp32 -- the wide-map scan BACKWARD of ss2d_w.hpp reads them without
// an unpack (its forward keeps the 16-bit rows: with five operand vectors per chunk row it is bound by the vector-memory path)
template <typename T>
__global__ void __launch_bounds__(256) route_split_kernel(const T *xd, T *xr, T *Bs, T *Cs, float *Bs32, float *Cs32, int R, int N,
                                                          int H, int W) {
    extern __shared__ float tile[];
    const int C2 = R + 2 * N, L = H * W;
    const int c = blockIdx.x % C2, bk = blockIdx.x / C2, k = bk & 3;
    const T *src = xd + (int64_t)blockIdx.x * L;
    const bool tr = (k & 1) != 0;
    if (c < R) {
        plane_move<T, T>(src, xr + ((int64_t)bk * R + c) * L, H, W, tr, tile);
        return;
    }
    const int64_t off = c < R + N ? ((int64_t)bk * N + (c - R)) * L : ((int64_t)bk * N + (c - R - N)) * L;
    T *dst = (c < R + N ? Bs : Cs) + off;
    if (!Bs32) {
        plane_move<T, T>(src, dst, H, W, tr, tile);
        return;
    }
    // both copies of the row in one pass over the source
    float *dst32 = (c < R + N ? Bs32 : Cs32) + off;
    if (!tr) {
        for (int e = threadIdx.x; e < L; e += blockDim.x) {
            const float v = ldf<T>(src + e);
            stf<T>(dst + e, v);
            dst32[e] = v;
        }
        return;
    }
    const int pitch = W + 1;
    for (int e = threadIdx.x; e < L; e += blockDim.x) {
        const int r = e / W, cc = e - r * W;
        tile[r * pitch + cc] = ldf<T>(src + e);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < L; e += blockDim.x) {     // (H x W) row-major -> (W x H) row-major
        const int cc = e / H, r = e - cc * H;
        const float v = tile[r * pitch + cc];
        stf<T>(dst + e, v);
        dst32[e] = v;
    }
}

// adjoint: gradients arrive as dt-input grad (T), dBs / dCs (fp32 accumulators of the scan backward)
template <typename T>
__global__ void __launch_bounds__(256) route_merge_kernel(const T *dxr, const float *dBs, const float *dCs, T *dxd, int R,
                                                          int N, int H, int W) {
    extern __shared__ float tile[];
    const int C2 = R + 2 * N, L = H * W;
    const int c = blockIdx.x % C2, bk = blockIdx.x / C2, k = bk & 3;
    T *dst = dxd + (int64_t)blockIdx.x * L;
    const bool tr = (k & 1) != 0;
    if (c < R) plane_move<T, T>(dxr + ((int64_t)bk * R + c) * L, dst, W, H, tr, tile);
    else if (c < R + N) plane_move<float, T>(dBs + ((int64_t)bk * N + (c - R)) * L, dst, W, H, tr, tile);
    else plane_move<float, T>(dCs + ((int64_t)bk * N + (c - R - N)) * L, dst, W, H, tr, tile);
}

template <typename T>
static int launch_route(bool merge, const void *a, const void *b, const void *c, void *d, void *e, void *f, int B, int R,
                        int N, int H, int W, hipStream_t s, float *e32 = nullptr, float *f32 = nullptr) {
    const size_t lds = (size_t)(H > W ? H : W) * ((H > W ? W : H) + 1) * sizeof(float) + (size_t)(H + W) * sizeof(float);
    if (lds > 64 * 1024) return XFM_ELIMIT;
    const dim3 grid((unsigned)((int64_t)B * 4 * (R + 2 * N)));
    if (merge)
        hipLaunchKernelGGL((route_merge_kernel<T>), grid, dim3(256), lds, s, (const T *)a, (const float *)b,
                           (const float *)c, (T *)d, R, N, H, W);
    else
        hipLaunchKernelGGL((route_split_kernel<T>), grid, dim3(256), lds, s, (const T *)a, (T *)d, (T *)e, (T *)f, e32, f32, R, N, H, W);
    return check_launch();
}

// ---- flexible routes (xfm_cross_scan_flex / xfm_cross_merge_flex) ----------------------------------------------
// Index maps of triton_cross_scan_flex (models/csm_triton.py:279-400): route k's position q for the map position
// p = h*W + w is
//   scans 0 (cross2d): q0 = p, q1 = w*H + h, q2 = L-1-q0, q3 = L-1-q1
//   scans 1 (unidi):   q0 = q1 = q2 = q3 = p
//   scans 2 (bidi):    q0 = q1 = p, q2 = q3 = L-1-p
// scan: y_k[q_k(p)] = x[p] (one_by_one: x_k[p]);  merge: x[p] = sum_k y_k[q_k(p)] in fp32 (one_by_one: x_k[p] = y_k[q_k(p)]).
// x is (B, C, L) channel-first or (B, L, C) channel-last, with a route axis (B, 4, C, L) / (B, L, 4, C) under one_by_one;
// y is (B, 4, C, L) or (B, L, 4, C).  Three kernels serve the configurations:
//   flex_rows_kernel   both sides channel-last: every route moves whole C-rows, vector loads / stores along C;
//   flex_planes_kernel both sides channel-first, no transposed route (scans 1/2): vector loads / stores along L, the
//                      flipped routes reverse the vector in registers;
//   flex_tile_kernel   everything else (layouts differ, or one_by_one cross2d channel-first): a (channels x rows x
//                      columns) tile staged in LDS, read and written with lanes along each side's contiguous axis.
// Scans move raw bits (Ti == To == uint16_t / float); merges convert through fp32 (Ti, To = float / f16_t / bf16_t).

template <typename T> struct Elt;
template <> struct Elt<float> {
    static __device__ __forceinline__ float get(float v) { return v; }
    static __device__ __forceinline__ float put(float v) { return v; }
};
template <> struct Elt<uint16_t> {  // 16-bit payload carried bit-exact through a 32-bit register / LDS word
    static __device__ __forceinline__ float get(uint16_t v) { return __uint_as_float(v); }
    static __device__ __forceinline__ uint16_t put(float v) { return (uint16_t)__float_as_uint(v); }
};
template <> struct Elt<bf16_t> {
    static __device__ __forceinline__ float get(bf16_t v) { return ldf<bf16_t>(&v); }
    static __device__ __forceinline__ bf16_t put(float v) { return __float2bfloat16(v); }
};
template <> struct Elt<f16_t> {
    static __device__ __forceinline__ float get(f16_t v) { return __half2float(v); }
    static __device__ __forceinline__ f16_t put(float v) { return __float2half(v); }
};

template <typename T, int V> struct alignas(sizeof(T) * V) Vec { T v[V]; };

__device__ __forceinline__ bool route_flipped(int k, int scans) { return scans != 1 && k >= 2; }
__device__ __forceinline__ bool route_transposed(int k, int scans) { return scans == 0 && (k & 1); }
__device__ __forceinline__ int64_t route_pos(int k, int scans, int h, int w, int H, int W) {
    const int64_t L = (int64_t)H * W;
    const int64_t q = route_transposed(k, scans) ? (int64_t)w * H + h : (int64_t)h * W + w;
    return route_flipped(k, scans) ? L - 1 - q : q;
}

// both sides channel-last; one item = V channels of one map position.  src / dst: x / y for the scan, y / x for the merge.
template <bool MERGE, typename Ti, typename To, int V>
__global__ void __launch_bounds__(256) flex_rows_kernel(const Ti *__restrict__ src, To *__restrict__ dst, int B, int C,
                                                        int H, int W, int obo, int scans) {
    const int64_t L = (int64_t)H * W, nv = C / V, total = (int64_t)B * L * nv;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
        const int64_t row = it / nv;
        const int ch = (int)(it - row * nv) * V;
        const int64_t b = row / L, p = row - b * L;
        const int h = (int)(p / W), w = (int)(p - (int64_t)h * W);
        const int64_t xrow = obo ? row * 4 * C + ch : row * C + ch;  // + k*C under one_by_one
        if (!MERGE) {
            Vec<Ti, V> v = *(const Vec<Ti, V> *)(src + xrow);
            for (int k = 0; k < 4; ++k) {
                if (obo && k) v = *(const Vec<Ti, V> *)(src + xrow + (int64_t)k * C);
                Vec<To, V> o;
#pragma unroll
                for (int i = 0; i < V; ++i) o.v[i] = Elt<To>::put(Elt<Ti>::get(v.v[i]));
                *(Vec<To, V> *)(dst + ((b * L + route_pos(k, scans, h, w, H, W)) * 4 + k) * C + ch) = o;
            }
        } else {
            float acc[V];
            for (int k = 0; k < 4; ++k) {
                const Vec<Ti, V> v = *(const Vec<Ti, V> *)(src + ((b * L + route_pos(k, scans, h, w, H, W)) * 4 + k) * C + ch);
#pragma unroll
                for (int i = 0; i < V; ++i) acc[i] = (obo || k == 0) ? Elt<Ti>::get(v.v[i]) : acc[i] + Elt<Ti>::get(v.v[i]);
                if (obo || k == 3) {
                    Vec<To, V> o;
#pragma unroll
                    for (int i = 0; i < V; ++i) o.v[i] = Elt<To>::put(acc[i]);
                    *(Vec<To, V> *)(dst + xrow + (obo ? (int64_t)k * C : 0)) = o;
                }
            }
        }
    }
}

// both sides channel-first, scans 1 or 2 (routes are the identity or a flip of L); one item = V positions of one plane.
template <bool MERGE, typename Ti, typename To, int V>
__global__ void __launch_bounds__(256) flex_planes_kernel(const Ti *__restrict__ src, To *__restrict__ dst, int B, int C,
                                                          int64_t L, int obo, int scans) {
    const int64_t nv = L / V, total = (int64_t)B * C * nv;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
        const int64_t plane = it / nv, p = (it - plane * nv) * V;
        const int64_t b = plane / C, c = plane - b * C;
        const int64_t xp = obo ? (b * 4 * C + c) * L + p : plane * L + p;  // + k*C*L under one_by_one
        auto yat = [&](int k) { return ((b * 4 + k) * C + c) * L + (route_flipped(k, scans) ? L - p - V : p); };
        if (!MERGE) {
            Vec<Ti, V> v = *(const Vec<Ti, V> *)(src + xp);
            for (int k = 0; k < 4; ++k) {
                if (obo && k) v = *(const Vec<Ti, V> *)(src + xp + (int64_t)k * C * L);
                const bool f = route_flipped(k, scans);
                Vec<To, V> o;
#pragma unroll
                for (int i = 0; i < V; ++i) o.v[i] = Elt<To>::put(Elt<Ti>::get(v.v[f ? V - 1 - i : i]));
                *(Vec<To, V> *)(dst + yat(k)) = o;
            }
        } else {
            float acc[V];
            for (int k = 0; k < 4; ++k) {
                const Vec<Ti, V> v = *(const Vec<Ti, V> *)(src + yat(k));
                const bool f = route_flipped(k, scans);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float e = Elt<Ti>::get(v.v[f ? V - 1 - i : i]);
                    acc[i] = (obo || k == 0) ? e : acc[i] + e;
                }
                if (obo || k == 3) {
                    Vec<To, V> o;
#pragma unroll
                    for (int i = 0; i < V; ++i) o.v[i] = Elt<To>::put(acc[i]);
                    *(Vec<To, V> *)(dst + xp + (obo ? (int64_t)k * C * L : 0)) = o;
                }
            }
        }
    }
}

// Tile walk orders: lanes along the columns (w), along the rows (h) or along the channels.  A channel-first side walks w
// for row-major positions and h for the column-major (transposed) routes; a channel-last side walks the channels.
enum { WALK_W = 0, WALK_H = 1, WALK_C = 2 };

template <int TC, int TH, int TW>
struct Tile {
    static constexpr int RP = TW + 1;            // odd row pitch: a walk along h is bank-conflict free
    static constexpr int CP = (TH * RP) | 1;     // odd channel pitch: a walk along the channels is bank-conflict free
    static constexpr int N = TC * TH * TW;
    struct Idx { int cc, hh, ww; };
    static __device__ __forceinline__ Idx at(int walk, int e) {
        if (walk == WALK_W) return {e / (TW * TH), (e / TW) % TH, e % TW};
        if (walk == WALK_H) return {e / (TH * TW), e % TH, (e / TH) % TW};
        return {e % TC, e / (TC * TW), (e / TC) % TW};
    }
};

template <bool MERGE, typename Ti, typename To, int TC, int TH, int TW>
__global__ void __launch_bounds__(256) flex_tile_kernel(const Ti *__restrict__ src, To *__restrict__ dst, int C, int H, int W,
                                                        int xcl, int ycl, int obo, int scans) {
    using T = Tile<TC, TH, TW>;
    __shared__ float S[TC * T::CP];
    const int ntw = (W + TW - 1) / TW;
    const int h0 = (blockIdx.x / ntw) * TH, w0 = (blockIdx.x % ntw) * TW, c0 = blockIdx.y * TC;
    const int64_t b = blockIdx.z, L = (int64_t)H * W;
    const int xwalk = xcl ? WALK_C : WALK_W;
    auto ywalk = [&](int k) { return ycl ? WALK_C : (route_transposed(k, scans) ? WALK_H : WALK_W); };
    // element offsets; the x route axis exists only under one_by_one
    auto xoff = [&](int k, int c, int h, int w) -> int64_t {
        const int64_t p = (int64_t)h * W + w;
        if (!obo) return xcl ? (b * L + p) * C + c : (b * C + c) * L + p;
        return xcl ? ((b * L + p) * 4 + k) * C + c : ((b * 4 + k) * C + c) * L + p;
    };
    auto yoff = [&](int k, int c, int h, int w) -> int64_t {
        const int64_t q = route_pos(k, scans, h, w, H, W);
        return ycl ? ((b * L + q) * 4 + k) * C + c : ((b * 4 + k) * C + c) * L + q;
    };
    // visit every in-range element of the tile in walk order: f(lds index, c, h, w)
    auto walk = [&](int order, auto f) {
        for (int e = threadIdx.x; e < T::N; e += 256) {
            const auto i = T::at(order, e);
            const int c = c0 + i.cc, h = h0 + i.hh, w = w0 + i.ww;
            if (c < C && h < H && w < W) f(i.cc * T::CP + i.hh * T::RP + i.ww, c, h, w);
        }
    };
    if (!MERGE) {
        for (int k = 0; k < 4; ++k) {
            if (k == 0 || obo) {
                if (k) __syncthreads();
                walk(xwalk, [&](int s, int c, int h, int w) { S[s] = Elt<Ti>::get(src[xoff(k, c, h, w)]); });
                __syncthreads();
            }
            walk(ywalk(k), [&](int s, int c, int h, int w) { dst[yoff(k, c, h, w)] = Elt<To>::put(S[s]); });
        }
    } else {
        for (int k = 0; k < 4; ++k) {
            const bool first = k == 0 || obo;
            walk(ywalk(k), [&](int s, int c, int h, int w) {
                const float v = Elt<Ti>::get(src[yoff(k, c, h, w)]);
                S[s] = first ? v : S[s] + v;
            });
            __syncthreads();
            if (obo || k == 3) {
                walk(xwalk, [&](int s, int c, int h, int w) { dst[xoff(k, c, h, w)] = Elt<To>::put(S[s]); });
                __syncthreads();
            }
        }
    }
}

static bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// widest vector (<= 16 bytes on either side) that divides n and that both base pointers are aligned for
template <typename Ti, typename To>
static int vec_width(int64_t n, const void *a, const void *b) {
    for (int v = 8; v > 1; v /= 2)
        if (v * sizeof(Ti) <= 16 && v * sizeof(To) <= 16 && n % v == 0 && aligned(a, v * sizeof(Ti)) &&
            aligned(b, v * sizeof(To)))
            return v;
    return 1;
}

static unsigned stride_grid(int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 256 * 32));
}

template <bool MERGE, typename Ti, typename To, int V>
static void launch_rows_v(const void *s, void *d, int B, int C, int H, int W, int obo, int scans, hipStream_t st) {
    hipLaunchKernelGGL((flex_rows_kernel<MERGE, Ti, To, V>), dim3(stride_grid((int64_t)B * H * W * (C / V))), dim3(256),
                       0, st, (const Ti *)s, (To *)d, B, C, H, W, obo, scans);
}

template <bool MERGE, typename Ti, typename To, int V>
static void launch_planes_v(const void *s, void *d, int B, int C, int64_t L, int obo, int scans, hipStream_t st) {
    hipLaunchKernelGGL((flex_planes_kernel<MERGE, Ti, To, V>), dim3(stride_grid((int64_t)B * C * (L / V))), dim3(256),
                       0, st, (const Ti *)s, (To *)d, B, C, L, obo, scans);
}

template <bool MERGE, typename Ti, typename To, int TC, int TH, int TW>
static void launch_tile(const void *s, void *d, int B, int C, int H, int W, int xcl, int ycl, int obo, int scans,
                        hipStream_t st) {
    const dim3 grid((unsigned)(((H + TH - 1) / TH) * ((W + TW - 1) / TW)), (unsigned)((C + TC - 1) / TC), (unsigned)B);
    hipLaunchKernelGGL((flex_tile_kernel<MERGE, Ti, To, TC, TH, TW>), grid, dim3(256), 0, st, (const Ti *)s, (To *)d, C, H,
                       W, xcl, ycl, obo, scans);
}

// s / d: x / y for the scan, y / x for the merge.  The channel-first cross2d configuration without one_by_one is the
// caller's (xfm_cross_scan / xfm_cross_merge).
template <bool MERGE, typename Ti, typename To>
static int launch_flex(const void *s, void *d, int B, int C, int H, int W, int xcl, int ycl, int obo, int scans,
                       hipStream_t st) {
    const int64_t L = (int64_t)H * W;
    if (xcl && ycl) {
        switch (vec_width<Ti, To>(C, s, d)) {
            case 8: launch_rows_v<MERGE, Ti, To, 8>(s, d, B, C, H, W, obo, scans, st); break;
            case 4: launch_rows_v<MERGE, Ti, To, 4>(s, d, B, C, H, W, obo, scans, st); break;
            case 2: launch_rows_v<MERGE, Ti, To, 2>(s, d, B, C, H, W, obo, scans, st); break;
            default: launch_rows_v<MERGE, Ti, To, 1>(s, d, B, C, H, W, obo, scans, st);
        }
    } else if (!xcl && !ycl && scans != 0) {
        switch (vec_width<Ti, To>(L, s, d)) {
            case 8: launch_planes_v<MERGE, Ti, To, 8>(s, d, B, C, L, obo, scans, st); break;
            case 4: launch_planes_v<MERGE, Ti, To, 4>(s, d, B, C, L, obo, scans, st); break;
            case 2: launch_planes_v<MERGE, Ti, To, 2>(s, d, B, C, L, obo, scans, st); break;
            default: launch_planes_v<MERGE, Ti, To, 1>(s, d, B, C, L, obo, scans, st);
        }
    } else if (!xcl && !ycl) {
        launch_tile<MERGE, Ti, To, 1, 64, 64>(s, d, B, C, H, W, xcl, ycl, obo, scans, st);  // plane transposes
    } else {
        launch_tile<MERGE, Ti, To, 16, 16, 16>(s, d, B, C, H, W, xcl, ycl, obo, scans, st);
    }
    return check_launch();
}

static bool flex_args_ok(const void *a, const void *b, int B, int C, int H, int W, int xl, int yl, int obo, int scans) {
    return a && b && B > 0 && C > 0 && H > 0 && W > 0 && (xl == 0 || xl == 1) && (yl == 0 || yl == 1) &&
           (obo == 0 || obo == 1) && scans >= 0 && scans <= 2 && B <= 65535 && (int64_t)H * W <= INT32_MAX;
}

}  // namespace xfm

extern "C" {

int xfm_ss2d_route_split(const void *xd, void *xr, void *Bs, void *Cs, int B, int R, int N, int H, int W, int dtype,
                         void *stream) {
    using namespace xfm;
    if (!xd || !xr || !Bs || !Cs || B <= 0 || R <= 0 || N <= 0 || H <= 0 || W <= 0) return XFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case XFM_F32: return launch_route<float>(false, xd, nullptr, nullptr, xr, Bs, Cs, B, R, N, H, W, s);
        case XFM_F16: return launch_route<f16_t>(false, xd, nullptr, nullptr, xr, Bs, Cs, B, R, N, H, W, s);
        case XFM_BF16: return launch_route<bf16_t>(false, xd, nullptr, nullptr, xr, Bs, Cs, B, R, N, H, W, s);
    }
    return XFM_EDTYPE;
}

int xfm_ss2d_route_split_bc32(const void *xd, void *xr, void *Bs, void *Cs, float *Bs32, float *Cs32, int B, int R, int N, int H,
                              int W, int dtype, void *stream) {
    using namespace xfm;
    if (!xd || !xr || !Bs || !Cs || !Bs32 || !Cs32 || B <= 0 || R <= 0 || N <= 0 || H <= 0 || W <= 0) return XFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case XFM_F32: return launch_route<float>(false, xd, nullptr, nullptr, xr, Bs, Cs, B, R, N, H, W, s, Bs32, Cs32);
        case XFM_F16: return launch_route<f16_t>(false, xd, nullptr, nullptr, xr, Bs, Cs, B, R, N, H, W, s, Bs32, Cs32);
        case XFM_BF16: return launch_route<bf16_t>(false, xd, nullptr, nullptr, xr, Bs, Cs, B, R, N, H, W, s, Bs32, Cs32);
    }
    return XFM_EDTYPE;
}

int xfm_ss2d_route_merge(const void *dxr, const float *dBs, const float *dCs, void *dxd, int B, int R, int N, int H,
                         int W, int dtype, void *stream) {
    using namespace xfm;
    if (!dxr || !dBs || !dCs || !dxd || B <= 0 || R <= 0 || N <= 0 || H <= 0 || W <= 0) return XFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case XFM_F32: return launch_route<float>(true, dxr, dBs, dCs, dxd, nullptr, nullptr, B, R, N, H, W, s);
        case XFM_F16: return launch_route<f16_t>(true, dxr, dBs, dCs, dxd, nullptr, nullptr, B, R, N, H, W, s);
        case XFM_BF16: return launch_route<bf16_t>(true, dxr, dBs, dCs, dxd, nullptr, nullptr, B, R, N, H, W, s);
    }
    return XFM_EDTYPE;
}

int xfm_cross_scan(const void *x, void *y, int B, int C, int H, int W, int dtype, void *stream) {
    using namespace xfm;
    if (!x || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return XFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case XFM_F32: return launch_scan<float>(x, y, B, C, H, W, s);
        case XFM_F16: return launch_scan<f16_t>(x, y, B, C, H, W, s);
        case XFM_BF16: return launch_scan<bf16_t>(x, y, B, C, H, W, s);
    }
    return XFM_EDTYPE;
}

int xfm_cross_merge(const void *y, void *x, int B, int C, int H, int W, int in_dtype, int out_dtype, void *stream) {
    using namespace xfm;
    if (!x || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0) return XFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (in_dtype == XFM_F32 && out_dtype == XFM_F32) return launch_merge<float, float>(y, x, B, C, H, W, s);
    if (in_dtype == XFM_F32 && out_dtype == XFM_BF16) return launch_merge<float, bf16_t>(y, x, B, C, H, W, s);
    if (in_dtype == XFM_F32 && out_dtype == XFM_F16) return launch_merge<float, f16_t>(y, x, B, C, H, W, s);
    if (in_dtype == XFM_BF16 && out_dtype == XFM_BF16) return launch_merge<bf16_t, bf16_t>(y, x, B, C, H, W, s);
    if (in_dtype == XFM_F16 && out_dtype == XFM_F16) return launch_merge<f16_t, f16_t>(y, x, B, C, H, W, s);
    if (in_dtype == XFM_BF16 && out_dtype == XFM_F32) return launch_merge<bf16_t, float>(y, x, B, C, H, W, s);
    if (in_dtype == XFM_F16 && out_dtype == XFM_F32) return launch_merge<f16_t, float>(y, x, B, C, H, W, s);
    return XFM_EDTYPE;
}

int xfm_swap_scan(const void *x, const void *x2, void *out, int B, int C, int L, int dtype, void *stream) {
    using namespace xfm;
    if (!x || !x2 || !out || B <= 0 || C <= 0 || L <= 0) return XFM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)B * C * L;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 8);
    switch (dtype) {
        case XFM_F32:
            hipLaunchKernelGGL((swap_scan_kernel<float>), dim3(grid), dim3(256), 0, s, (const float *)x,
                               (const float *)x2, (float *)out, total, C, L);
            break;
        case XFM_F16:
        case XFM_BF16:
            hipLaunchKernelGGL((swap_scan_kernel<uint16_t>), dim3(grid), dim3(256), 0, s, (const uint16_t *)x,
                               (const uint16_t *)x2, (uint16_t *)out, total, C, L);
            break;
        default: return XFM_EDTYPE;
    }
    return check_launch();
}

int xfm_cross_scan_flex(const void *x, void *y, int B, int C, int H, int W, int x_layout, int y_layout, int one_by_one,
                        int scans, int dtype, void *stream) {
    using namespace xfm;
    if (!flex_args_ok(x, y, B, C, H, W, x_layout, y_layout, one_by_one, scans)) return XFM_EINVAL;
    if (dtype != XFM_F32 && dtype != XFM_F16 && dtype != XFM_BF16) return XFM_EDTYPE;
    if (!x_layout && !y_layout && !one_by_one && scans == 0) return xfm_cross_scan(x, y, B, C, H, W, dtype, stream);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == XFM_F32) return launch_flex<false, float, float>(x, y, B, C, H, W, x_layout, y_layout, one_by_one, scans, s);
    return launch_flex<false, uint16_t, uint16_t>(x, y, B, C, H, W, x_layout, y_layout, one_by_one, scans, s);
}

int xfm_cross_merge_flex(const void *y, void *x, int B, int C, int H, int W, int x_layout, int y_layout, int one_by_one,
                         int scans, int in_dtype, int out_dtype, void *stream) {
    using namespace xfm;
    if (!flex_args_ok(y, x, B, C, H, W, x_layout, y_layout, one_by_one, scans)) return XFM_EINVAL;
    if (!x_layout && !y_layout && !one_by_one && scans == 0)
        return xfm_cross_merge(y, x, B, C, H, W, in_dtype, out_dtype, stream);
    hipStream_t s = (hipStream_t)stream;
    const int a = x_layout, b = y_layout, o = one_by_one;
#define XFM_MERGE_FLEX(I, O, TI, TO) \
    if (in_dtype == I && out_dtype == O) return launch_flex<true, TI, TO>(y, x, B, C, H, W, a, b, o, scans, s);
    XFM_MERGE_FLEX(XFM_F32, XFM_F32, float, float)
    XFM_MERGE_FLEX(XFM_F32, XFM_BF16, float, bf16_t)
    XFM_MERGE_FLEX(XFM_F32, XFM_F16, float, f16_t)
    XFM_MERGE_FLEX(XFM_BF16, XFM_BF16, bf16_t, bf16_t)
    XFM_MERGE_FLEX(XFM_F16, XFM_F16, f16_t, f16_t)
    XFM_MERGE_FLEX(XFM_BF16, XFM_F32, bf16_t, float)
    XFM_MERGE_FLEX(XFM_F16, XFM_F32, f16_t, float)
#undef XFM_MERGE_FLEX
    return XFM_EDTYPE;
}
}
