// The SLSTM of Encodec (SLSTM.cs:31,40-57): the persistent layer kernel with its cross-workgroup exchange of h, the step-wise fallback,
// the per-device ticket that serialises the persistent sections of different handles, and the launch sequence (layers in sequence, or
// layer-pipelined over two streams).  Arithmetic is the canonical arithmetic of DESIGN.md (same sequences as oracle/c/nc_ref_encodec.c).
#include <algorithm>
#include <cstdio>
#include <mutex>

#include "nc_math.h"
#include "nc_model.h"

namespace nc {

// ---------------------------------------------------------------------------------------------- kernels
// One LSTM time step of one layer (SLSTM.cs:31,40-57; gate order i,f,g,o).  Block j = hidden unit, thread = clip.
//   gi   [B,4C,T]  input projection incl. b_ih (matrix-core 1x1 conv)         hprev/hnext, cst  [C][B] (unit-major)
//   out  [B,C,T]   h_t (+ skip[b,j,t] for the last layer: output.add(permuted), SLSTM.cs:50-53; elu_out: the ELU every consumer of an
//                  SLSTM applies first -- SEANetEncoder.cs / SEANetDecoder.cs: [.., SLSTM, ELU, conv] -- is applied here, once)
__global__ __launch_bounds__(64) void lstm_step_kernel(const float* __restrict__ gi, const float* __restrict__ whh,
                                                       const float* __restrict__ bhh, const float* __restrict__ hprev,
                                                       float* __restrict__ hnext, float* __restrict__ cst, const float* __restrict__ skip,
                                                       float* __restrict__ out, int B, int C, int64_t T, int64_t t, int elu_out) {
    extern __shared__ float wrow[];   // [4][C]
    const int j = blockIdx.x;
    for (int i = threadIdx.x; i < 4 * C; i += 64) wrow[i] = whh[(int64_t)((i / C) * C + j) * C + (i % C)];
    __syncthreads();
    const int b = blockIdx.y * 64 + threadIdx.x;
    if (b >= B) return;
    // recurrent contraction: four quarter chains combined as (q0 + q1) + (q2 + q3) (the canonical order: oracle slstm); one chain
    // when C is not a multiple of 4
    float r0, r1, r2, r3;
    {
        const int nq = (C % 4 == 0) ? 4 : 1, qlen = C / nq;
        float q0[4], q1[4], q2[4], q3[4];
        for (int s4 = 0; s4 < nq; ++s4) {
            float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
            for (int k = s4 * qlen; k < (s4 + 1) * qlen; ++k) {
                const float h = hprev[(int64_t)k * B + b];
                c0 = nc_fma(wrow[k], h, c0);
                c1 = nc_fma(wrow[C + k], h, c1);
                c2 = nc_fma(wrow[2 * C + k], h, c2);
                c3 = nc_fma(wrow[3 * C + k], h, c3);
            }
            q0[s4] = c0; q1[s4] = c1; q2[s4] = c2; q3[s4] = c3;
        }
        if (nq == 4) {
            r0 = (q0[0] + q0[1]) + (q0[2] + q0[3]);
            r1 = (q1[0] + q1[1]) + (q1[2] + q1[3]);
            r2 = (q2[0] + q2[1]) + (q2[2] + q2[3]);
            r3 = (q3[0] + q3[1]) + (q3[2] + q3[3]);
        } else {
            r0 = q0[0]; r1 = q1[0]; r2 = q2[0]; r3 = q3[0];
        }
    }
    const float* g = gi + ((int64_t)b * 4 * C) * T + t;
    const float pi = g[(int64_t)j * T] + (r0 + bhh[j]);
    const float pf = g[(int64_t)(C + j) * T] + (r1 + bhh[C + j]);
    const float pg = g[(int64_t)(2 * C + j) * T] + (r2 + bhh[2 * C + j]);
    const float po = g[(int64_t)(3 * C + j) * T] + (r3 + bhh[3 * C + j]);
    const float ig = nc_sigmoidf(pi), fg = nc_sigmoidf(pf), gg = nc_tanhf(pg), og = nc_sigmoidf(po);
    const float cn = (fg * cst[(int64_t)j * B + b]) + (ig * gg);
    cst[(int64_t)j * B + b] = cn;
    const float h = og * nc_tanhf(cn);
    hnext[(int64_t)j * B + b] = h;
    const int64_t o = ((int64_t)b * C + j) * T + t;
    const float y = skip ? h + skip[o] : h;
    out[o] = elu_out ? nc_eluf(y) : y;
}

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const void* lstm_gptr;
typedef __attribute__((address_space(3))) void* lstm_lptr;

// Persistent LSTM layer: ALL T time steps of one layer in ONE launch (SLSTM.cs:31,40-57).
//   * W_hh stays in LDS for the whole sequence: a workgroup of 16 wavefronts owns 16 hidden units; wave (ub, q) holds the 16 gate
//     rows of 4 units (one 16-row matrix-core tile) for quarter q of the reduction: 128 KB per workgroup at C = 512 -- one workgroup
//     per CU, C/16 workgroups per 16-clip column tile, loaded once by LDS DMA.
//   * Per step the recurrent contraction runs as FOUR quarter chains (the canonical order of the oracle: (q0 + q1) + (q2 + q3)) walked
//     side by side by the four waves of a unit block: the dependent chain -- the critical path of the step -- is 32
//     v_mfma_f32_16x16x4_f32 instead of 128 (0.5 us instead of 2.1); the partial tiles meet in LDS and the q = 0 wave applies the gates
//     with the cell state in its registers.
//   * h_t of a column tile is exchanged between its C/16 workgroups through global memory with the placement-independent
//     release/acquire protocol of cdna_hip_programming.md G16 (recipe R1): write-through (sc1) payload stores -> vmcnt(0) ->
//     workgroup barrier -> one relaxed agent-scope flag store per workgroup; consumers poll the flags of their tile (one lane per
//     producer, relaxed), a workgroup barrier, and then read the h tile with relaxed AGENT-SCOPE (sc1) loads, which bypass the CU's L1
//     and observe the producers' write-through stores directly -- the shipped build has NO acquire fence (the "sc1 stores and sc1
//     loads both sides" form of MI355X_MICROARCH.md; ordering between the flag and the payload comes from the producer's vmcnt(0)
//     drain before its flag store and the consumer's barrier before its loads).  NC_SYNC_ACQUIRE=1 adds the acquire fence behind the poll
//     at run time (an operational fallback, exercised by tests/test_children_gpu.py); -DNC_LSTM_FENCE is the compile-time fence +
//     plain-load variant (`make CXXFLAGS+=-DNC_LSTM_FENCE`; no envmatrix row builds it).  Layout [unit][16 clips] = the B-fragment order: every operand load is a 256-byte row.  Double-buffered by step parity: a
//     workgroup can only publish h_{t+1} after every workgroup of the tile has published h_t, i.e. finished reading h_{t-1}.
//   * Every spin is bounded: a timeout sets *tmo and all workgroups leave (the host reports NC_EDEVICE at the next synchronise).
// Grid = (C/16, column tiles): at most 128 workgroups of 140 KB LDS per launch, all co-resident on the 256 CUs.
// (A granule form of the exchange -- 8-byte {tag, value} stores, data-is-flag -- measured slower: 18.1 vs 17.0 ms on C3.)
struct LstmSeqArgs {
    const float* gi;      // [N,4C,T] input projections incl. b_ih
    const float* whhp;    // [C/4 unit blocks][KS][64] A-fragment image of W_hh
    const float* bhh;     // [4C]
    const float* skip;    // nullable [N,C,T]: added to the last layer's output (SLSTM.cs:50-53)
    float* out;           // [N,C,T]
    int elu_out;          // ELU applied to the stored value (the activation in front of the consuming convolution)
    float* hx;            // [2][tiles][C][16] exchange buffers
    unsigned* flags;      // [tiles][C/16] steps published per workgroup (zeroed before the launch)
    unsigned* tmo;        // timeout word (zeroed at model creation)
    float* cstate;        // [tiles][C][16] cell state carried between the chunk launches of one layer
    // element strides of gi / out over (clip, channel row, step): [N][rows][T] = (rows*T, T, 1) for tensors that meet the convolution
    // stack, [rows][T][N] = (1, T*N, N) for the tensors between the layers of a pipelined call (a step range is then a contiguous
    // column range of one 2-D matrix, which is what the chunked input-projection GEMM of the next layer wants)
    int64_t gi_b, gi_c, gi_t, out_b, out_c, out_t;
    int N, C;
    int64_t T;
    int64_t t0, t1;       // this launch runs steps [t0, t1) of the T-step sequence (state of step t0-1 in hx / cstate / flags)
    int tile0;            // first column tile of this launch
    int acquire;          // NC_SYNC_ACQUIRE=1: agent-scope acquire fence behind the flag poll (the textbook hand-off; the default reads h with
                          // agent-scope loads of drained write-through stores instead: validated by the parity sweeps and run in both forms by
                          // tests/test_children_gpu.py)
};
typedef __attribute__((address_space(1))) unsigned lstm_gu32;
// UB = unit blocks (of 4 hidden units) per workgroup: 4 (16 wavefronts, C/16 workgroups per column tile) or 2 (8 wavefronts, C/8
// workgroups per tile: two chains per SIMD instead of four -- the matrix-core part of a step halves, twice the CUs take part)
// HT (round 6, the default; NC_LSTM_NO_HTILE=1 selects the form above): the h tile goes through LDS and the weights live in REGISTERS.
//   The four unit-block waves of a quarter need the same 8 KB of h_{t-1}; each fetched it for itself -- 128 KB of agent-scope reads per
//   workgroup and step, a good part of the step's ~1.5 us operand fetch at the CU's fabric port.  Now the 16 waves fetch the 32 KB tile
//   ONCE (8 coalesced dword reads per lane, the same agent-scope loads), park it in LDS, and every wave takes its 32 B fragments from
//   there; W_hh (a wave's share is QS x 64 words = 32 registers) stays in registers for the whole sequence instead of being re-read from
//   LDS every step.  One more workgroup barrier per step; same operands, same chains: bit-identical.
template <int KS, int UB = 4, bool HT = true>
__global__ __launch_bounds__(256 * UB, 1) void lstm_seq_kernel(const LstmSeqArgs a) {
    constexpr int QS = KS / 4;                                          // k-steps per quarter
    constexpr int CC = 4 * KS;                                          // hidden units (= a.C)
    extern __shared__ __attribute__((aligned(16))) float lstm_lds[];   // [4 UB waves][QS][64] weights (HT: [CC][16] h tile) | [3][UB][64] f32x4 partial tiles
    __shared__ int dead;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ubl = wave % UB, q = wave / UB;       // unit block within the workgroup, reduction quarter
    const int C = a.C, N = a.N;
    const int64_t T = a.T;
    const int nprod = C / (4 * UB);                 // workgroups per column tile
    const int ubw = blockIdx.x, tile = blockIdx.y;  // tile: local index within this launch
    const int ub = ubw * UB + ubl;                   // unit block of this wave: hidden units 4*ub .. 4*ub+3
    float* Aw = lstm_lds + wave * QS * 64;
    float* const Hs = lstm_lds;
    f32x4v* const part = reinterpret_cast<f32x4v*>(lstm_lds + (HT ? CC * 16 : 4 * UB * QS * 64));
    const float* wsrc = a.whhp + ((int64_t)ub * KS + q * QS) * 64;
    float aw[HT ? QS : 1];
    if constexpr (HT) {
#pragma unroll
        for (int i = 0; i < QS; ++i) aw[i] = wsrc[i * 64 + lane];
    } else {
#pragma unroll
        for (int i = 0; i < QS / 4; ++i)
            __builtin_amdgcn_global_load_lds((lstm_gptr)(wsrc + i * 256 + lane * 4), (lstm_lptr)(Aw + i * 256), 16, 0, 0);
    }
    if (threadIdx.x == 0) dead = 0;
    const int k4 = lane >> 4, cl = lane & 15;
    const int j = ub * 4 + k4;                      // this lane's hidden unit
    const int b = (a.tile0 + tile) * 16 + cl;       // this lane's clip
    const int bb = min(b, N - 1);
    const float* g = a.gi + (int64_t)bb * a.gi_b;
    const int64_t gc = a.gi_c, gt = a.gi_t;
    const float bh0 = a.bhh[j], bh1 = a.bhh[C + j], bh2 = a.bhh[2 * C + j], bh3 = a.bhh[3 * C + j];
    float* const hx0 = a.hx + ((int64_t)(0 * gridDim.y + tile) * C) * 16;
    float* const hx1 = a.hx + ((int64_t)(1 * gridDim.y + tile) * C) * 16;
    unsigned* const flags = a.flags + (int64_t)tile * nprod;
    const int64_t orow = ((int64_t)bb * C + j) * T;                       // skip tensor: always [N,C,T]
    float* const orow_out = a.out + (int64_t)bb * a.out_b + (int64_t)j * a.out_c;
    float* const cs_slot = a.cstate + ((int64_t)tile * C) * 16 + ub * 64 + lane;
    float cst = (q == 0 && a.t0 > 0) ? *cs_slot : 0.0f;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // input-projection pre-activations (and the skip value) run one step ahead of their use (q = 0 waves only): they are reads,
    // issued before the step's stores, so they never queue behind a store acknowledgement
    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f, sk = 0.0f;
    if (q == 0) {
        const int64_t ts = a.t0;
        g0 = g[(int64_t)j * gc + ts * gt]; g1 = g[(int64_t)(C + j) * gc + ts * gt]; g2 = g[(int64_t)(2 * C + j) * gc + ts * gt]; g3 = g[(int64_t)(3 * C + j) * gc + ts * gt];
        if (a.skip) sk = a.skip[orow + ts];
    }
    for (int64_t t = a.t0; t < a.t1; ++t) {
        f32x4v acc = {0.0f, 0.0f, 0.0f, 0.0f};
        const float c0 = g0, c1 = g1, c2 = g2, c3 = g3, csk = sk;
        const int64_t tn = min(t + 1, T - 1);
        if (t > 0) {                                 // h_{-1} = 0: every quarter chain of step 0 is +0
            if (wave == 0) {
                const unsigned want = (unsigned)t;
                bool ok = false;
                for (unsigned spins = 0; spins < (1u << 21); ++spins) {
                    const unsigned v = lane < nprod ? __hip_atomic_load((lstm_gu32*)(flags + lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
                    if (__all(v >= want)) { ok = true; break; }
                    if ((spins & 1023) == 1023 && __hip_atomic_load((lstm_gu32*)a.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!ok && lane == 0) {
                    __hip_atomic_store((lstm_gu32*)a.tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    dead = 1;
                }
#ifdef NC_LSTM_FENCE
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#else
                if (a.acquire) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
            }
            __syncthreads();
            if (dead) return;
            float hb[QS];
            // the h operands are read with agent-scope (sc1) loads: they observe the producers' write-through stores directly, so the
            // consumer needs no acquire fence (an agent-scope L1 invalidation costs ~1.7 us, more than the loads themselves)
            if constexpr (HT) {
                constexpr int NT = 256 * UB, NL = (CC * 16 + NT - 1) / NT;
                const float* hsrc = (t & 1) ? hx0 : hx1;                 // h_{t-1} sits in buffer (t-1)&1: [unit][16 clips], CC * 16 words
                float hv[NL];
#pragma unroll
                for (int u = 0; u < NL; ++u) {
                    const int idx = min(u * NT + (int)threadIdx.x, CC * 16 - 1);
#ifdef NC_LSTM_FENCE
                    hv[u] = hsrc[idx];
#else
                    hv[u] = __hip_atomic_load(hsrc + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
                }
                if (q == 0) {
                    g0 = g[(int64_t)j * gc + tn * gt]; g1 = g[(int64_t)(C + j) * gc + tn * gt]; g2 = g[(int64_t)(2 * C + j) * gc + tn * gt]; g3 = g[(int64_t)(3 * C + j) * gc + tn * gt];
                    if (a.skip) sk = a.skip[orow + tn];
                }
#pragma unroll
                for (int u = 0; u < NL; ++u)
                    if (u * NT + (int)threadIdx.x < CC * 16) Hs[u * NT + threadIdx.x] = hv[u];
                __syncthreads();
#pragma unroll
                for (int i = 0; i < QS; ++i) hb[i] = Hs[(q * QS + i) * 64 + lane];
#pragma unroll
                for (int i = 0; i < QS; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[i], hb[i], acc, 0, 0, 0);
            } else {
                const float* hp = ((t & 1) ? hx0 : hx1) + (int64_t)q * QS * 64 + lane;   // h_{t-1} sits in buffer (t-1)&1
#pragma unroll
                for (int i = 0; i < QS; ++i) {
#ifdef NC_LSTM_FENCE
                    hb[i] = hp[i * 64];
#else
                    hb[i] = __hip_atomic_load(hp + i * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
                }
                if (q == 0) {
                    g0 = g[(int64_t)j * gc + tn * gt]; g1 = g[(int64_t)(C + j) * gc + tn * gt]; g2 = g[(int64_t)(2 * C + j) * gc + tn * gt]; g3 = g[(int64_t)(3 * C + j) * gc + tn * gt];
                    if (a.skip) sk = a.skip[orow + tn];
                }
#pragma unroll
                for (int i = 0; i < QS; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Aw[i * 64 + lane], hb[i], acc, 0, 0, 0);
            }
            if (q > 0) part[((q - 1) * UB + ubl) * 64 + lane] = acc;
            __syncthreads();
            if (q == 0) {
                const f32x4v p1 = part[(0 * UB + ubl) * 64 + lane], p2 = part[(1 * UB + ubl) * 64 + lane], p3 = part[(2 * UB + ubl) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = (acc[r] + p1[r]) + (p2[r] + p3[r]);
            }
        } else if (q == 0) {
            g0 = g[(int64_t)j * gc + tn * gt]; g1 = g[(int64_t)(C + j) * gc + tn * gt]; g2 = g[(int64_t)(2 * C + j) * gc + tn * gt]; g3 = g[(int64_t)(3 * C + j) * gc + tn * gt];
            if (a.skip) sk = a.skip[orow + tn];
        }
        if (q == 0) {
            const float pi = c0 + (acc[0] + bh0);
            const float pf = c1 + (acc[1] + bh1);
            const float pg = c2 + (acc[2] + bh2);
            const float po = c3 + (acc[3] + bh3);
            const float ig = nc_sigmoidf(pi), fg = nc_sigmoidf(pf), gg = nc_tanhf(pg), og = nc_sigmoidf(po);
            cst = (fg * cst) + (ig * gg);
            const float h = og * nc_tanhf(cst);
            if (t + 1 < T) {
                // publish h_t: write-through payload, drained per wave, then one flag store for the workgroup
                float* hq = ((t & 1) ? hx1 : hx0) + ub * 64 + lane;   // [unit j][clip cl] = j*16 + cl = ub*64 + lane
                __hip_atomic_store(hq, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            if (b < N) {
                const float yo = a.skip ? h + csk : h;
                orow_out[t * a.out_t] = a.elu_out ? nc_eluf(yo) : yo;
            }
        }
        if (t + 1 < T) {
            __syncthreads();   // the four publishing waves have drained their stores (and the partial tiles are free again)
            if (threadIdx.x == 0) __hip_atomic_store((lstm_gu32*)(flags + ubw), (unsigned)(t + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (q == 0 && a.t1 < T) *cs_slot = cst;   // the next chunk launch of this layer resumes from here
}

// [N][C][T] -> [C][T][N]: the layout in which a range of steps is one contiguous column range (the chunked input projections of the layer-pipelined form)
__global__ void nct_to_ctn_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int C, int64_t T) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * C * T) return;
    const int n = (int)(i % N);
    const int64_t r = i / N, t = r % T, c = r / T;
    y[i] = x[((int64_t)n * C + c) * T + t];
}

// ---------------------------------------------------------------------------------------------- weights
void load_lstm(const Blob& b, const std::string& key, Lstm& l, int C, int n_layers) {
    l.C = C;
    l.layers.clear();
    for (int i = 0; i < n_layers; ++i) {
        l.layers.emplace_back(new LstmLayer());
        LstmLayer& y = *l.layers.back();
        char sfx[32];
        snprintf(sfx, sizeof sfx, "_l%d", i);
        const BlobTensor& wih = b.get(key + ".lstm.weight_ih" + sfx);
        const BlobTensor& whh = b.get(key + ".lstm.weight_hh" + sfx);
        const BlobTensor& bih = b.get(key + ".lstm.bias_ih" + sfx);
        const BlobTensor& bhh = b.get(key + ".lstm.bias_hh" + sfx);
        if (wih.numel() != (int64_t)4 * C * C || whh.numel() != (int64_t)4 * C * C || bih.numel() != 4 * C || bhh.numel() != 4 * C)
            fail(NC_EINVAL, "%s: LSTM tensors have the wrong shape", key.c_str());
        y.ih.kclass = NC_KC_CONV_K1;
        y.ih.build(static_cast<const float*>(wih.data), static_cast<const float*>(bih.data), C, 4 * C, 1, 1, 0, 1, 0, false);
        upload_f32(y.whh, static_cast<const float*>(whh.data), (size_t)4 * C * C);
        if (C % 4 == 0) {   // A-fragment image for lstm_seq_kernel: [unit block][k-step][lane], lane = (k4 << 4) | (unit << 2) | gate
            const float* w = static_cast<const float*>(whh.data);
            std::vector<float> pk((size_t)4 * C * C);
            const int KS = C / 4;
            for (int ub = 0; ub < C / 4; ++ub)
                for (int kp = 0; kp < KS; ++kp)
                    for (int l = 0; l < 64; ++l) {
                        const int k4 = l >> 4, r = l & 15, u = r >> 2, gate = r & 3;
                        pk[((size_t)ub * KS + kp) * 64 + l] = w[(size_t)(gate * C + ub * 4 + u) * C + 4 * kp + k4];
                    }
            upload_f32(y.whhp, pk.data(), pk.size());
        }
        upload_f32(y.bhh, static_cast<const float*>(bhh.data), (size_t)4 * C);
        upload_f32(y.bih, static_cast<const float*>(bih.data), (size_t)4 * C);
    }
}

bool lstm_applies_elu(const Lstm& l) {
    static const bool off = env_flag("NC_LSTM_NO_ELU");
    return !off && !l.layers.empty();
}

// ---- per-device ticket of the persistent LSTM sections (include/nc_mi355x.h "threading": distinct handles may run concurrently) --------
// A persistent launch needs ALL its workgroups resident (one per CU at ~140 KB of LDS); a handle budgets its own launches for that (<= 64
// workgroups per launch, two pipelined layers, a concurrent tail-segment group: <= 192 of the 256 CUs).  Two handles driven from two host
// threads on ONE device would double that: partially resident launches then spin for CUs that other partially resident launches hold, until
// the bounded spins time out and both handles drop to the step-wise kernels for good.  So the LSTM sections of DIFFERENT handles on one
// device run one after the other on the GPU: a section waits for the event recorded behind the previous section (of any handle) and
// records it again behind itself -- stream-ordered, no host wait; the mutex only keeps two host threads from interleaving their enqueues
// (held for the ~100 us a section takes to enqueue).  A device with one LSTM-running handle never waits.  Everything else of the two
// handles (convolutions, quantizer) still overlaps.  Other PROCESSES on the same device are outside its reach (the timeout path remains).
struct LstmTicket {
    std::mutex mu;
    hipEvent_t ev = nullptr;   // behind the last persistent section enqueued on this device
    int live = 0;              // handles on this device that have run a persistent section
    const void* last_owner = nullptr;   // the handle's runtime that recorded `ev`
};
static LstmTicket& lstm_ticket_of(int device) {
    // (leaked on purpose: handles destroyed during static destruction still find their ticket -- ADVICE r5)
    static std::mutex* m = new std::mutex();
    static std::map<int, LstmTicket*>* t = new std::map<int, LstmTicket*>();
    std::lock_guard<std::mutex> lk(*m);
    LstmTicket*& p = (*t)[device];
    if (!p) p = new LstmTicket();
    return *p;
}
struct LstmSection {
    LstmTicket& t;
    LstmRuntime& r;
    hipStream_t s;
    std::unique_lock<std::mutex> lk;
    int unwinding_at_entry;
    LstmSection(LstmRuntime& rt, hipStream_t stream)
        : t(rt.ticket ? *rt.ticket : lstm_ticket_of(rt.m.device)), r(rt), s(stream), lk(t.mu), unwinding_at_entry(std::uncaught_exceptions()) {
        if (!r.ticket) { r.ticket = &t; ++t.live; }
        if (!t.ev) NC_HIP(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
        // (with more than one live handle EVERY section waits for the one before it, a handle's own included: the event is re-recorded by
        //  each section, so the chain main group -> side group -> next handle is what keeps a third party behind all of them)
        else if (t.live > 1) NC_HIP(hipStreamWaitEvent(s, t.ev, 0));
    }
    ~LstmSection() {
        if (!t.ev) return;
        if (std::uncaught_exceptions() > unwinding_at_entry) {
            // error path: the layer-pipelined form may have left persistent launches on the second stream that were never joined into `s`;
            // the ticket must not be handed on before they are done
            if (r.stream2) (void)hipStreamSynchronize(r.stream2);
            (void)hipStreamSynchronize(s);
        }
        (void)hipEventRecord(t.ev, s);
        t.last_owner = &r;
    }
};

// ---------------------------------------------------------------------------------------------- runtime
void LstmRuntime::prepare() {
    if (tmo_host) return;
    void* hp = nullptr;
    NC_HIP(hipHostMalloc(&hp, 64, hipHostMallocMapped));
    std::memset(hp, 0, 64);
    tmo_host = static_cast<unsigned*>(hp);
    void* dp = nullptr;
    NC_HIP(hipHostGetDevicePointer(&dp, hp, 0));
    tmo_dev = static_cast<unsigned*>(dp);
}

LstmRuntime::~LstmRuntime() {
    if (stream2) (void)hipStreamDestroy(stream2);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (tmo_host) (void)hipHostFree(tmo_host);
    if (ticket) {
        std::lock_guard<std::mutex> lk(ticket->mu);
        --ticket->live;
        if (ticket->last_owner == this) ticket->last_owner = nullptr;
        if (ticket->live == 0 && ticket->ev) {   // (the last handle of the device: the event goes with it; the next first section makes a new one)
            (void)hipEventDestroy(ticket->ev);
            ticket->ev = nullptr;
        }
    }
}

bool LstmRuntime::note_timeout() {
    if (!timed_out()) return false;
    // the launches of the failed call that are still queued could raise the word again after it has been cleared: let them finish first
    // (every side stream of a call joins the handle's stream before the call returns, so this covers them)
    (void)hipStreamSynchronize(m.stream);
    *reinterpret_cast<volatile unsigned*>(tmo_host) = 0;
    force_stepwise = true;
    ++timeouts;
    return true;
}

// The persistent kernel needs every workgroup of a launch resident at once (one per CU at 140 KB of LDS): up to 64 per launch, two
// launches in flight when the layers are pipelined, beside a concurrent segment group.  Devices (or partitions) that cannot hold
// that, and handles that have seen a timeout, take the step-wise kernels.
static bool persistent_ok(const LstmRuntime& r, int C) {
    static const bool stepwise_env = env_flag("NC_LSTM_STEPWISE");
    const int KS = C / 4;
    const size_t lds_need = (size_t)4 * KS * 64 * 4 + 3 * 4 * 64 * 16;
    const bool stepwise = stepwise_env || r.force_stepwise || r.m.cu_count < 192 || r.m.lds_per_cu < lds_need + 1024;
    return !stepwise && C % 64 == 0 && (KS == 128 || KS == 16);
}

// W_ih * x_t + b_ih for all steps: one pointwise convolution over the [N,C,T] tensor
static void ih_gemm(EncodecModel& m, LstmLayer& y, const float* in, float* gi, int N, int C, int64_t T) {
    ConvIO io{};
    io.x = in; io.x_bstride = (int64_t)C * T; io.x_cstride = T; io.x_len = (int32_t)T; io.Tin = T;
    io.y = gi; io.y_bstride = (int64_t)4 * C * T; io.y_cstride = T;
    launch_conv(y.ih, io, N, m.stream, &m.prof);
}

// Chunk boundaries (even: chunk starts stay 8-byte aligned for the 1x1 path).  The layer above trails the layer below by its
// LAST chunk (+ that chunk's input-projection GEMM), so the last chunk is short (T/8) and the others share the rest: with 4
// chunks of 150 steps 44 / 44 / 44 / 18 instead of 38 / 38 / 38 / 36 (6 chunks: 28 / 28 / 28 / 28 / 20 / 18) -- the tail after layer 0 has finished shrinks from 36
// steps to 18 without a single extra cross-stream event.
std::vector<int64_t> lstm_chunk_starts(int64_t T, int n_layers, int want_chunks, bool even_chunks, bool may_pipe) {
    std::vector<int64_t> cstart{0};
    if (n_layers >= 2 && want_chunks > 1 && T >= 32 && may_pipe) {
        const int64_t last = even_chunks ? 0 : std::max<int64_t>(8, (T / 8) & ~(int64_t)1);
        const int nbig = even_chunks ? want_chunks : want_chunks - 1;
        int64_t big = ((((T - last) + nbig - 1) / nbig) + 1) & ~(int64_t)1;
        big = std::max<int64_t>(big, 8);
        for (int64_t t0 = big; t0 < ((T - last) & ~(int64_t)1); t0 += big) cstart.push_back(t0);
        const int64_t tail0 = (T - last) & ~(int64_t)1;   // an even start whatever the parity of T: the last chunk absorbs the odd step
        if (last > 0 && tail0 > cstart.back()) cstart.push_back(tail0);
    }
    cstart.push_back(T);
    return cstart;
}

// One persistent call: its geometry and the buffers of its layers.
struct LstmCall {
    const float* x;                 // [N,C,T] input of the stack (the skip of its last layer)
    int N, C, nl, n_tiles, UBW, nprod, per_launch;
    int64_t T;
    bool elu_out, piped;
    size_t lds, ev_i = 0;
    std::vector<int64_t> cstart;    // chunk k runs steps [cstart[k], cstart[k + 1])
    std::vector<float*> gi, out, hx, cs;
    std::vector<unsigned*> flags;
    hipStream_t sA, sB;             // streams of the even / odd layers
    int nch() const { return (int)cstart.size() - 1; }
    hipStream_t layer_stream(int li) const { return (li & 1) ? sB : sA; }
    // tensor of layer li that sits between two pipelined layers ([rows][T][N]) instead of meeting the convolution stack ([N][rows][T])
    bool between(int li_out) const { return piped && li_out + 1 < nl; }
};

// Persistent layer kernel: a launch runs a range of steps for a group of column tiles (<= 64 co-resident workgroups, so the
// two layers of a pipelined call plus a concurrent segment group still fit the chip's 256 CUs at one workgroup per CU).
// Layer pipelining: layer l+1 at step t needs only h^l_t, so the sequence is cut into chunks and chunk k of layer l+1 (with its
// input-projection GEMM) runs on a second stream while layer l runs chunk k+1: the dependent chain of a 2-layer LSTM shrinks
// from 2T steps to about T + T/chunks.  The arithmetic is untouched -- the same kernel, resumed from carried (h, c) state.
// The tensors BETWEEN the layers (h^l and the input projections of layer l+1) are laid out [rows][T][N]: the steps of a chunk
// are then one contiguous column range of a 2-D matrix, so the chunk's GEMM is a one-"clip" pointwise convolution over
// chunk*N columns with full 128-column tiles (cut out of [N,C,T], a chunk would fill a fifth of every tile: measured, the
// per-chunk GEMMs then cost as much as the full one and 6 chunks made C3 2.2 ms slower).
// (round 6: 6 chunks, was 4 -- re-swept after the projection GEMMs moved to the pointwise kernel: C3 8.26 -> 8.21 ms, Encodec 24 kHz x 16 clips
//  5.51 -> 5.26 ms; 8 chunks: back to the 4-chunk times.  tools/probe/r6_chunks24.sh)
static LstmCall plan_persistent(EncodecModel& m, Lstm& l, const float* x, int N, int64_t T, bool elu_out) {
    static const int want_chunks = [] { const int v = (int)env_int("NC_LSTM_CHUNKS", 6); return v < 1 ? 1 : v; }();
    static const bool even_chunks = env_flag("NC_LSTM_EVEN_CHUNKS");
    LstmCall c;
    const int C = l.C, KS = C / 4, nl = (int)l.layers.size();
    c.x = x; c.N = N; c.C = C; c.nl = nl; c.T = T; c.elu_out = elu_out;
    c.cstart = lstm_chunk_starts(T, nl, want_chunks, even_chunks, !m.on_side_group && (int64_t)4 * C * T * N < ((int64_t)1 << 31));
    c.piped = c.nch() > 1;
    // Unit blocks per workgroup: 2 at C = 512 with ONE column tile (64 workgroups of 8 wavefronts, 72 KB of LDS each -- the
    // matrix-core part of a step is 2 chains per SIMD instead of 4: 1.8 -> 0.9 us of the ~5.7; Encodec 24 kHz at 16 clips
    // 6.24 -> 6.13 ms), 4 otherwise: with two tiles the 2 x 64-producer exchange costs more than the chains save (C3 9.59 -> 9.70 ms).
    // NC_LSTM_UB=4 / 2 force one form.
    static const int ub_env = (int)env_int("NC_LSTM_UB", 0);
    c.n_tiles = (N + 15) / 16;
    c.UBW = (KS == 128 && (ub_env == 2 || (ub_env != 4 && c.n_tiles == 1))) ? 2 : 4;
    c.nprod = C / (4 * c.UBW);
    c.per_launch = std::max(1, (c.UBW == 2 ? 128 : 64) / c.nprod);
    c.lds = (size_t)4 * c.UBW * (KS / 4) * 64 * 4 + 3 * c.UBW * 64 * 16;
    c.gi.resize(nl); c.out.resize(nl); c.hx.resize(nl); c.cs.resize(nl); c.flags.resize(nl);
    for (int li = 0; li < nl; ++li) {
        c.gi[li] = m.alloc((size_t)N * 4 * C * T);
        c.out[li] = m.alloc((size_t)N * C * T);
        c.cs[li] = m.alloc((size_t)c.n_tiles * C * 16);
        c.hx[li] = m.alloc((size_t)2 * c.n_tiles * C * 16);
        c.flags[li] = reinterpret_cast<unsigned*>(m.alloc((size_t)c.n_tiles * c.nprod));   // per call + layer: groups may run concurrently
        NC_HIP(hipMemsetAsync(c.flags[li], 0, (size_t)c.n_tiles * c.nprod * 4, m.stream));
    }
    c.sA = c.sB = m.stream;
    return c;
}

static hipEvent_t next_event(LstmRuntime& r, LstmCall& c) {
    if (c.ev_i == r.events.size()) {
        r.events.push_back(nullptr);
        NC_HIP(hipEventCreateWithFlags(&r.events.back(), hipEventDisableTiming));
    }
    return r.events[c.ev_i++];
}

// the instance for KS = C / 4 k-steps, UBW unit blocks per workgroup and the LDS h tile (HT) or the form before it
typedef void (*LstmSeqKernel)(const LstmSeqArgs);
static LstmSeqKernel lstm_seq_instance(int KS, int UBW, bool htile) {
    if (KS == 128 && UBW == 2) return htile ? lstm_seq_kernel<128, 2, true> : lstm_seq_kernel<128, 2, false>;
    if (KS == 128) return htile ? lstm_seq_kernel<128, 4, true> : lstm_seq_kernel<128, 4, false>;
    return htile ? lstm_seq_kernel<16, 4, true> : lstm_seq_kernel<16, 4, false>;
}

// steps [t0, t1) of layer li on its stream: one launch per group of `per_launch` column tiles
static void launch_chunk(LstmRuntime& r, const LstmCall& c, Lstm& l, int li, int64_t t0, int64_t t1) {
    Profiler& prof = r.m.prof;
    static const bool sync_acquire = env_flag("NC_SYNC_ACQUIRE");
    static const bool no_htile = env_flag("NC_LSTM_NO_HTILE");   // every wave fetches its own h operands, W_hh in LDS (the round-2..5 form)
    LstmLayer& y = *l.layers[li];
    hipStream_t s = c.layer_stream(li);
    const bool last = li + 1 == c.nl;
    const int N = c.N, C = c.C;
    const int64_t T = c.T;
    const double n = (double)N * (double)(t1 - t0);
    const LstmSeqKernel kern = lstm_seq_instance(C / 4, c.UBW, !no_htile);
    if (prof.on) prof.begin(s, NC_KC_LSTM, 2.0 * 4 * C * C * n, 4.0 * 6 * C * n);
    for (int tl = 0; tl < c.n_tiles; tl += c.per_launch) {
        const int nt = std::min(c.per_launch, c.n_tiles - tl);
        LstmSeqArgs a{};
        a.gi = c.gi[li]; a.whhp = y.whhp.as<float>(); a.bhh = y.bhh.as<float>(); a.skip = last ? c.x : nullptr; a.out = c.out[li]; a.elu_out = (last && c.elu_out) ? 1 : 0;
        if (c.piped) { a.gi_b = 1; a.gi_c = T * N; a.gi_t = N; }
        else { a.gi_b = (int64_t)4 * C * T; a.gi_c = T; a.gi_t = 1; }
        if (c.between(li)) { a.out_b = 1; a.out_c = T * N; a.out_t = N; }
        else { a.out_b = (int64_t)C * T; a.out_c = T; a.out_t = 1; }
        a.hx = c.hx[li] + (size_t)2 * tl * C * 16;
        a.cstate = c.cs[li] + (size_t)tl * C * 16;
        a.flags = c.flags[li] + (size_t)tl * c.nprod; a.tmo = r.tmo_dev;   // timeout word (host-visible)
        a.N = N; a.C = C; a.T = T; a.t0 = t0; a.t1 = t1; a.tile0 = tl;
        a.acquire = sync_acquire ? 1 : 0;
        ensure_dynamic_lds((const void*)kern, c.lds);
        hipLaunchKernelGGL(kern, dim3((unsigned)c.nprod, (unsigned)nt), dim3(256 * c.UBW), c.lds, s, a);
    }
    NC_HIP(hipGetLastError());
    if (prof.on) prof.end(s);
}

// the input projections of chunk k of a layer: columns [t0*N, (t0+n)*N) of the [rows][T*N] matrices
static void ih_gemm_chunk(EncodecModel& m, const LstmCall& c, LstmLayer& y, const float* in, float* g, int k, hipStream_t s) {
    const int64_t t0 = c.cstart[(size_t)k], n = c.cstart[(size_t)k + 1] - t0, TN = c.T * c.N;
    ConvIO io{};
    io.x = in + t0 * c.N; io.x_bstride = 0; io.x_cstride = TN; io.x_len = (int32_t)(n * c.N); io.Tin = n * c.N;
    io.y = g + t0 * c.N; io.y_bstride = 0; io.y_cstride = TN;
    launch_conv(y.ih, io, 1, s, &m.prof);
}

// The layer-pipelined schedule.
// Layer 0's input projections depend on x alone: x goes to the [C][T][N] layout once and its chunk GEMMs run ahead on the second
// stream, chunk k releasing layer 0's chunk k (the recurrence starts after the first chunk's GEMM, not after the whole one).
// The projection GEMM of chunk k of a layer ABOVE runs on the stream of the layer BELOW, right behind that layer's chunk k:
// the layer above then runs its chunks back to back (on its own stream, GEMM and chunk alternating, it was the sum of both --
// ~1.0 ms for 0.78 ms of recurrence -- and bounded the whole LSTM), while the layer below, which finishes a short last chunk
// ahead anyway, absorbs the ~40 us per GEMM.  (A third stream for the GEMMs measured WORSE: the runtime multiplexes streams onto
// 4 hardware queues, the extra stream shared a queue with the tail-segment group or the other layer and serialised with it,
// +0.9 ms; with GPU_MAX_HW_QUEUES=8 every queue got slower gaps, +1.8 ms.)
static void run_piped(LstmRuntime& r, LstmCall& c, Lstm& l) {
    EncodecModel& m = r.m;
    const int N = c.N, C = c.C, nch = c.nch();
    const int64_t T = c.T;
    if (!r.stream2) NC_HIP(hipStreamCreateWithFlags(&r.stream2, hipStreamNonBlocking));
    c.sB = r.stream2;
    {
        hipEvent_t fork = next_event(r, c);
        NC_HIP(hipEventRecord(fork, c.sA));
        NC_HIP(hipStreamWaitEvent(c.sB, fork, 0));
    }
    std::vector<hipEvent_t> ready(nch, nullptr);   // ready[k]: the input projections of chunk k of the current layer are complete
    {
        float* xT = m.alloc((size_t)N * C * T);
        const int64_t n = (int64_t)N * C * T;
        hipLaunchKernelGGL(nct_to_ctn_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.sB, c.x, xT, N, C, T);
        NC_HIP(hipGetLastError());
        for (int k = 0; k < nch; ++k) {
            ih_gemm_chunk(m, c, *l.layers[0], xT, c.gi[0], k, c.sB);
            ready[k] = next_event(r, c);
            NC_HIP(hipEventRecord(ready[k], c.sB));
        }
    }
    for (int li = 0; li < c.nl; ++li) {
        hipStream_t s = c.layer_stream(li);
        for (int k = 0; k < nch; ++k) {
            NC_HIP(hipStreamWaitEvent(s, ready[k], 0));
            launch_chunk(r, c, l, li, c.cstart[(size_t)k], c.cstart[(size_t)k + 1]);
            if (li + 1 < c.nl) {
                ih_gemm_chunk(m, c, *l.layers[li + 1], c.out[li], c.gi[li + 1], k, s);
                ready[k] = next_event(r, c);
                NC_HIP(hipEventRecord(ready[k], s));
            }
        }
    }
    hipEvent_t join = next_event(r, c);   // the handle's stream continues after everything issued on the second one
    NC_HIP(hipEventRecord(join, c.sB));
    NC_HIP(hipStreamWaitEvent(c.sA, join, 0));
}

static float* run_persistent(LstmRuntime& r, Lstm& l, const float* x, int N, int64_t T, bool elu_out) {
    LstmSection section(r, r.m.stream);   // (see LstmTicket: sections of different handles on one device run one after the other)
    LstmCall c = plan_persistent(r.m, l, x, N, T, elu_out);
    {   // NC_LSTM_FAKE_TIMEOUT=1 (tests): the first persistent launch of the process is reported as timed out
        static bool fake = env_flag("NC_LSTM_FAKE_TIMEOUT");
        if (fake) { fake = false; *reinterpret_cast<volatile unsigned*>(r.tmo_host) = 1; }
    }
    if (FILE* lf = launch_log()) {   // the form of the call, for tests/test_encodec_layers_gpu.py
        static const bool no_htile = env_flag("NC_LSTM_NO_HTILE");
        std::fprintf(lf, "lstm seq C=%d UBW=%d htile=%d piped=%d chunks=%d tiles=%d layers=%d T=%lld\n", c.C, c.UBW, no_htile ? 0 : 1, c.piped ? 1 : 0, c.nch(),
                     c.n_tiles, c.nl, (long long)T);
        std::fflush(lf);
    }
    if (c.piped) run_piped(r, c, l);
    else
        for (int li = 0; li < c.nl; ++li) {
            ih_gemm(r.m, *l.layers[li], li ? c.out[li - 1] : x, c.gi[li], N, c.C, T);
            launch_chunk(r, c, l, li, 0, T);
        }
    return c.out[c.nl - 1];
}

// One layer of the step-wise form on steps [0, T): the input projections of `in`, then one fresh launch per time step (block = hidden
// unit with its 4 weight rows in LDS, thread = clip) from the state in (h0, cs) -- [C][N], unit-major; h1 is the other half of the
// double-buffered h.  Returns the half that holds h_T.  No workgroup waits for another: a step is ordered behind the one before it by
// the stream alone.  (nc_lstm.h)
float* lstm_layer_steps(EncodecModel& m, LstmLayer& y, int C, const float* in, const float* skip, float* out, float* h0, float* h1, float* cs, int N, int64_t T,
                        bool elu_out) {
    hipStream_t stream = m.stream;
    float* gi = m.alloc((size_t)N * 4 * C * T);
    ih_gemm(m, y, in, gi, N, C, T);
    if (m.prof.on) m.prof.begin(stream, NC_KC_LSTM, 2.0 * 4 * C * C * (double)N * T, 4.0 * 6 * C * (double)N * T);
    for (int64_t t = 0; t < T; ++t)
        hipLaunchKernelGGL(lstm_step_kernel, dim3((unsigned)C, (unsigned)((N + 63) / 64)), dim3(64), (size_t)4 * C * sizeof(float), stream,
                           gi, y.whh.as<float>(), y.bhh.as<float>(), (t & 1) ? h1 : h0, (t & 1) ? h0 : h1, cs, skip, out, N, C, T, t, elu_out ? 1 : 0);
    NC_HIP(hipGetLastError());
    if (m.prof.on) m.prof.end(stream);
    return (T & 1) ? h1 : h0;
}

// generic fallback: one launch per time step, from the zero state
static float* run_stepwise(EncodecModel& m, Lstm& l, const float* x, int N, int64_t T, bool elu_out) {
    const int C = l.C, nl = (int)l.layers.size();
    hipStream_t stream = m.stream;
    if (FILE* lf = launch_log()) {
        std::fprintf(lf, "lstm step C=%d layers=%d T=%lld\n", C, nl, (long long)T);
        std::fflush(lf);
    }
    const float* in = x;
    float* out = nullptr;
    for (int li = 0; li < nl; ++li) {
        const bool last = li + 1 == nl;
        out = m.alloc((size_t)N * C * T);
        float* h0 = m.alloc((size_t)C * N);
        float* h1 = m.alloc((size_t)C * N);
        float* cs = m.alloc((size_t)C * N);
        NC_HIP(hipMemsetAsync(h0, 0, (size_t)C * N * 4, stream));
        NC_HIP(hipMemsetAsync(cs, 0, (size_t)C * N * 4, stream));
        lstm_layer_steps(m, *l.layers[li], C, in, last ? x : nullptr, out, h0, h1, cs, N, T, last && elu_out);
        in = out;
    }
    return out;
}

float* LstmRuntime::run(Lstm& l, const float* x, int N, int64_t T, bool elu_out) {
    if (l.layers.empty()) return const_cast<float*>(x);
    return persistent_ok(*this, l.C) ? run_persistent(*this, l, x, N, T, elu_out) : run_stepwise(m, l, x, N, T, elu_out);
}

}  // namespace nc
