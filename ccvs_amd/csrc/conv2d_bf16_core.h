// The arithmetic that the two large-tile forms of the split-bf16 convolution share: the per-tile producer / consumer kernel
// (conv2d_bf16x3_pc_kernel, conv2d_bf16_kernels.h) and the persistent-tiles kernel (conv2d_bf16x3_pt_kernel, conv2d_bf16_pt.h)
// give the same bits because both expand THESE definitions -- the MFMA order per output, the hi / lo split and the epilogue's add
// order exist once.  Each piece takes as parameters exactly what differs between the two kernels:
//   OFF     the LDS offset of tap column tb inside a tap row, a function-like macro: `xd0 + tb * xdd` (per tile: a tap table) or
//           `tb` (persistent: always the dense 3 x 3)
//   TID     the thread id of the epilogue's store phase: `tid`, or the persistent kernel's opaque copy `tid_`
//   STRIDE  threads that share a pass of the fp32 epilogue (512)
//   BIAS    the bias value of an output channel: the per-tile kernel holds its workgroup's 32 MB values (`bias_s`), the
//           persistent one the whole layer's (`bias_all`)
//   OK / OPIX / CLAMP  the bounds guard of an item of the packed epilogue, its pixel offset (0 where the guard fails) and the clamp
//           of its addend's channel: the per-tile packed epilogue also serves ragged tiles, the persistent kernel's tiles are
//           whole (OK = true, the plain offset, CLAMP = CB_NO_CLAMP)
// The pieces are macros on purpose: they expand between the register arrays, barriers and scheduling fences of kernels whose
// instruction streams hipcc changes at the slightest provocation (the comments below record the cases), and a macro is the same
// text at both sites by construction.  The K tail and the accumulator stage were tried as __forceinline__ templates taking the
// arrays by reference: both changed the instruction streams of the kernels that use them (profiles/conv_shared_core.txt), so they
// are macros too.  Names an expansion site must have in scope are listed per piece.
#pragma once
#include "common.h"
#include "conv_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// the 16-byte stores of the epilogues
__device__ __forceinline__ void cb_store16(void* dst, f32x4 v) { *reinterpret_cast<f32x4*>(dst) = v; }
__device__ __forceinline__ void cb_store16(void* dst, uint4 v) { cb_store16(dst, f32x4{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)}); }

#define CB_NO_CLAMP(c) (c)
// workgroup barrier behind an LDS-only wait: global stores / loads stay in flight (__syncthreads() also drains vmcnt)
#define CB_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// ---- the 512-pixel tap (PP = 4) --------------------------------------------------------------------------------------------
// Four pixel blocks of a tap stay in registers (fq); the weight fragments of the tap's MB output-channel blocks sit in one of
// two sets (fw): the next tap's are read above the current tap's 12 MB MFMAs (callers unroll the tap loop by two so that the
// sets stay statically indexed).  There is no second set for the pixels: in the pass over the LAST channel block each pixel
// block is re-read for the next tap right after its last MFMA -- 9 to 0 MFMAs before the next tap needs it, the
// earliest-needed block first.
// In scope: bf16x8 fq[4][2], fw[2][MB][2]; acc, bofs, it0, wt0 (the step's tap row of the halo tile / the weights), plane, NT, MB.
#define CB_TAP4_PRIME(OFF)                                                                                             \
    {                                                                                                                  \
        _Pragma("unroll") for (int pp = 0; pp < 4; ++pp) {                                                             \
            fq[pp][0] = __builtin_bit_cast(bf16x8, it0[OFF(0) + bofs[pp]]);                                            \
            fq[pp][1] = __builtin_bit_cast(bf16x8, it0[OFF(0) + plane + bofs[pp]]);                                    \
        }                                                                                                              \
        _Pragma("unroll") for (int m = 0; m < MB; ++m) {                                                               \
            fw[0][m][0] = __builtin_bit_cast(bf16x8, wt0[m * 32]);                                                     \
            fw[0][m][1] = __builtin_bit_cast(bf16x8, wt0[NT + m * 32]);                                                \
        }                                                                                                              \
    }
#define CB_TAP4(CUR, tb, more, OFF)                                                                                    \
    {                                                                                                                  \
        const uint4* itn_ = it0 + OFF((tb) + 1);                                                                       \
        if (more) {                                                                                                    \
            const uint4* wtn_ = wt0 + ((tb) + 1) * 4 * NT;                                                             \
            _Pragma("unroll") for (int m = 0; m < MB; ++m) {                                                           \
                fw[(CUR) ^ 1][m][0] = __builtin_bit_cast(bf16x8, wtn_[m * 32]);                                        \
                fw[(CUR) ^ 1][m][1] = __builtin_bit_cast(bf16x8, wtn_[NT + m * 32]);                                   \
            }                                                                                                          \
        }                                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        _Pragma("unroll") for (int m = 0; m < MB; ++m) {                                                               \
            _Pragma("unroll") for (int pp = 0; pp < 4; ++pp) {                                                         \
                acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[CUR][m][1], fq[pp][0], acc[m][pp], 0, 0, 0);   \
                acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[CUR][m][0], fq[pp][1], acc[m][pp], 0, 0, 0);   \
                acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[CUR][m][0], fq[pp][0], acc[m][pp], 0, 0, 0);   \
                if (m == MB - 1 && (more)) {                                                                           \
                    fq[pp][0] = __builtin_bit_cast(bf16x8, itn_[bofs[pp]]);                                            \
                    fq[pp][1] = __builtin_bit_cast(bf16x8, itn_[plane + bofs[pp]]);                                    \
                }                                                                                                      \
            }                                                                                                          \
        }                                                                                                              \
    }

// ---- the 256-pixel tap (PP = 2), software-pipelined -------------------------------------------------------------------------
// The ds_reads of the NEXT 32-cout block (and, on a tap's last block, of the next tap's pixels) are issued before the current
// block's 6 MFMAs, into the other register set -- hipcc does not do this by itself and the lone MFMA wave of a SIMD then idles
// a full LDS latency after every 6 MFMAs.  Taps are unrolled by two so both sets stay statically indexed.
// 3 x 3 kernels (three taps per row, known at compile time) write the tap loop out -- CB_LD_B(0, 0) CB_LD_A(0, 0, 0)
// CB_TAP(0, 0, 0, true) CB_TAP(1, (MB & 1), 1, true) CB_TAP(0, 0, 2, false) --, so that no run-time branch sits between the
// fragment reads and the MFMAs.  In the loop form hipcc's wait-count pass puts `s_waitcnt lgkmcnt(0)` directly behind every
// prefetch (`ds_read x2; s_waitcnt lgkmcnt(0); v_mfma x6`: it waits for the reads it has JUST issued); written out, the waits
// sit 4-6 MFMAs behind the reads (+1...+3 % per shape).  Hand-counted waits with the reads as asm statements were tried and
// are 2.4 x SLOWER: with an LDS-DMA in flight (the next step's weights) hipcc drains vmcnt in front of every asm statement
// that might touch LDS.
// In scope: bf16x8 fa[2][2] ([set][0 hi | 1 lo]: weights of one 32-cout block), fb[2][2][2] ([set][pp][0 hi | 1 lo]: the two
// pixel blocks of one tap); acc, bofs, it0, wt0, plane, NT, MB.
#define CB_LD_B(SET, tb, OFF)                                                                   \
    {                                                                                           \
        const uint4* it_ = it0 + OFF(tb);                                                       \
        _Pragma("unroll") for (int pp = 0; pp < 2; ++pp) {                                      \
            fb[SET][pp][0] = __builtin_bit_cast(bf16x8, it_[bofs[pp]]);                         \
            fb[SET][pp][1] = __builtin_bit_cast(bf16x8, it_[plane + bofs[pp]]);                 \
        }                                                                                       \
    }
#define CB_LD_A(SET, tb, m_)                                                                    \
    {                                                                                           \
        const uint4* wt_ = wt0 + (tb) * 4 * NT + (m_) * 32;                                     \
        fa[SET][0] = __builtin_bit_cast(bf16x8, wt_[0]);                                        \
        fa[SET][1] = __builtin_bit_cast(bf16x8, wt_[NT]);                                       \
    }
#define CB_TAP(BSET, A0, tb, has_next, OFF)                                                     \
    _Pragma("unroll") for (int m = 0; m < MB; ++m) {                                            \
        if (m + 1 < MB) {                                                                       \
            CB_LD_A(((A0) + m + 1) & 1, tb, m + 1)                                              \
        } else if (has_next) {                                                                  \
            CB_LD_A(((A0) + m + 1) & 1, (tb) + 1, 0)                                            \
            CB_LD_B((BSET) ^ 1, (tb) + 1, OFF)                                                  \
        }                                                                                       \
        __builtin_amdgcn_sched_barrier(0); /* keep the prefetch ABOVE the MFMAs it is meant to hide under */ \
        _Pragma("unroll") for (int pp = 0; pp < 2; ++pp) {                                      \
            acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[((A0) + m) & 1][1], fb[BSET][pp][0], acc[m][pp], 0, 0, 0); \
            acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[((A0) + m) & 1][0], fb[BSET][pp][1], acc[m][pp], 0, 0, 0); \
            acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[((A0) + m) & 1][0], fb[BSET][pp][0], acc[m][pp], 0, 0, 0); \
        }                                                                                       \
    }

// ---- the packed K tail (ccvs_conv_desc.w_ktail) ---------------------------------------------------------------------------
// The last chunk holds r = Cin % 16 <= 3 real channels.  Its nine taps x r channels are contracted in ceil(9 r / 16) MFMA
// steps whose K index runs over (tap, channel): position q = 16 j + 8 khalf + i of step j is tap q / r, channel q % r.  The
// weights arrive in that order (tap slots 0 .. nj-1 of tap row 0 of the chunk, at WTL: this lane's fragment of the step's weight
// buffer); the pixel operand is gathered from the chunk's staged tile (IH: the halo buffer as bf16), 2 bytes per (tap, channel)
// -- once per tile, against 9 - nj tap steps of 6 MB MFMAs saved.  Expanded OUTSIDE the step loop on purpose: inside it hipcc
// hoists the gather's address arithmetic over the whole loop and spills.
// In scope: acc, bofs, khalf, p (p.ktail = r), IWS, plane, NT, MB, PP.
#define CB_KTAIL(IH, WTL)                                                                                              \
    {                                                                                                                  \
        const int r_ = p.ktail, nq_ = 9 * r_, nj_ = (nq_ + 15) >> 4;                                                   \
        const unsigned short* ih = IH;                                                                                 \
        const uint4* wtl = WTL;                                                                                        \
        for (int j = 0; j < nj_; ++j) {                                                                                \
            bf16x8 gb[PP][2];                                                                                          \
            _Pragma("unroll") for (int pp = 0; pp < PP; ++pp) {                                                        \
                unsigned hw[4], lw[4];                                                                                 \
                _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                        \
                    const int q = 16 * j + 8 * khalf + i;                                                              \
                    const int qc = min(q, nq_ - 1);                                                                    \
                    const int t = qc / r_, c = qc - t * r_;                                                            \
                    const int tyy = t / 3, txx = t - 3 * tyy;                                                          \
                    const int e = (bofs[pp] + tyy * IWS + txx) * 8 + c; /* bf16 index inside the [pixel][8] plane */   \
                    unsigned hv = ih[e], lv = ih[plane * 8 + e];                                                       \
                    if (q >= nq_) { hv = 0; lv = 0; }                                                                  \
                    if (i & 1) { hw[i >> 1] |= hv << 16; lw[i >> 1] |= lv << 16; }                                     \
                    else { hw[i >> 1] = hv; lw[i >> 1] = lv; }                                                         \
                }                                                                                                      \
                gb[pp][0] = __builtin_bit_cast(bf16x8, make_uint4(hw[0], hw[1], hw[2], hw[3]));                        \
                gb[pp][1] = __builtin_bit_cast(bf16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));                        \
            }                                                                                                          \
            _Pragma("unroll") for (int m = 0; m < MB; ++m) {                                                           \
                const bf16x8 ah = __builtin_bit_cast(bf16x8, wtl[j * 4 * NT + m * 32]);                                \
                const bf16x8 al = __builtin_bit_cast(bf16x8, wtl[j * 4 * NT + NT + m * 32]);                           \
                _Pragma("unroll") for (int pp = 0; pp < PP; ++pp) {                                                    \
                    acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, gb[pp][0], acc[m][pp], 0, 0, 0);          \
                    acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, gb[pp][1], acc[m][pp], 0, 0, 0);          \
                    acc[m][pp] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, gb[pp][0], acc[m][pp], 0, 0, 0);          \
                }                                                                                                      \
            }                                                                                                          \
        }                                                                                                              \
    }

// ---- accumulators -> LDS stage ---------------------------------------------------------------------------------------------
// Dense convolutions: the accumulators of a 32-channel pass (one pixel column per lane, 16 couts in registers) go through LDS
// so that ALL 8 waves write 16-byte pieces along x (a lane then owns 4 consecutive pixels of one channel) instead of 128 scalar
// stores per consumer lane: the store tail was issue-bound.
// fp32 output: channel-major, [32 channels][NPIX].  Packed output: [pixel][32 channels] (36 floats apart: conflict-free
// 16-byte accesses) -- a lane writes its four groups of 4 consecutive channels as ds_write_b128, a reader fetches the 8
// channels of its pixel as two ds_read_b128 (channel-major staging cost the packed epilogue 8 ds_read_b32 per item: the
// 128-channel producers ran 20 % slower than with fp32 output).
// ACC: the pass's PP blocks of one MFMA wave (acc[m]); RW, LANE, KHALF: the wave in its role, the lane, lane >> 5 (the persistent
// kernel passes opaque copies).  In scope: stage, NPIX, PP.
#define CB_STAGE_PASS(ACC, P8, RW, LANE, KHALF)                                                                        \
    if (P8) {                                                                                                          \
        _Pragma("unroll") for (int pp = 0; pp < PP; ++pp) {                                                            \
            float* sp = stage + (((RW) * PP + pp) * 32 + ((LANE) & 31)) * 36 + 4 * (KHALF);                            \
            _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                            \
                const f32x4 q4 = {ACC[pp][4 * g], ACC[pp][4 * g + 1], ACC[pp][4 * g + 2], ACC[pp][4 * g + 3]};         \
                *reinterpret_cast<f32x4*>(sp + 8 * g) = q4;                                                            \
            }                                                                                                          \
        }                                                                                                              \
    } else {                                                                                                           \
        _Pragma("unroll") for (int pp = 0; pp < PP; ++pp)                                                              \
            _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                             \
                stage[((r & 3) + 8 * (r >> 2) + 4 * (KHALF)) * NPIX + ((RW) * PP + pp) * 32 + ((LANE) & 31)] = ACC[pp][r]; \
    }

// ---- the fast fp32 epilogue of a staged pass -------------------------------------------------------------------------------
// The whole tile inside the image, every output channel real, every row 16-byte aligned (the layers that matter), at most one
// addend: straight-line code -- hipcc can then COUNT its waits (vmcnt(n) for the addend of piece i leaves the stores of the
// pieces before it in flight; behind a per-piece branch it falls back to vmcnt(0)).
// No wait on vector memory inside the store loop: `s_waitcnt vmcnt` counts stores too, so a wait for a load issued after a
// store -- the bias value, the residual of the next piece -- also waits until that store has been acknowledged by memory
// (~0.6 us).  With the loads of every piece interleaved with its store the tile's 131 KB left the CU one round trip at a time:
// 9.9 us per 128-channel tile (timing ablations), a quarter of the time a 49->128 tile takes.  So the bias values come from
// LDS; a layer without addends (most of them) runs a code path of its own that issues no load at all (a load that is merely
// conditional still makes hipcc wait, vmcnt(0), where its value would be used), the others fetch the addend of ALL pieces of
// the pass first.  The offsets are recomputed where they are used: kept in arrays across the two phases they cost the
// 32-channel kernels, capped at 128 registers, a spill.
// add_kind (conv_add_kind): 0 none, 1 pre-activation image, 2 residual, 3 accumulate.
// In scope: stage, p, m, n0, tx, ty, TW, TH, NPIX, NIT (pieces per thread), add_kind, and of the image n: float* ybase,
// const float* abase with its channel stride a_sC (the one addend).
#define CB_EPI_OFFS(i, TID, STRIDE)                                                                  \
    const int idx4_ = TID + (STRIDE) * (i);                                                          \
    const int col_ = idx4_ / (NPIX / 4), px_ = (idx4_ % (NPIX / 4)) * 4;                             \
    const int prow_ = px_ / TW, pcol_ = px_ - prow_ * TW;                                            \
    const long opix_ = (long)(ty * TH + prow_) * p.Wout + tx * TW + pcol_;                           \
    const int co_ = n0 + m * 32 + col_;
#define CB_EPI_FINISH(ADD1, ADD2, ADD3, TID, STRIDE, BIAS)                                           \
_Pragma("unroll") for (int i = 0; i < NIT; ++i) {                                                    \
    CB_EPI_OFFS(i, TID, STRIDE)                                                                      \
    const float4 a4 = *reinterpret_cast<const float4*>(stage + col_ * NPIX + px_);                  \
    float v[4] = {a4.x, a4.y, a4.z, a4.w};                                                           \
    const float bv = BIAS;                                                                           \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                  \
        float t = (v[j] + (ADD1)) + bv;                                                              \
        if (p.act == CCVS_ACT_LRELU) t = lrelu01(t);                                                 \
        t = (t + (ADD2)) * p.out_scale;                                                              \
        v[j] = t + (ADD3);                                                                           \
    }                                                                                                \
    cb_store16(ybase + (long)co_ * p.out_sC + opix_, f32x4{v[0], v[1], v[2], v[3]});               \
}
#define CB_EPI_FAST(TID, STRIDE, BIAS)                                                               \
    if (add_kind == 0) {                                                                             \
        CB_EPI_FINISH(0.f, 0.f, 0.f, TID, STRIDE, BIAS)                                              \
    } else {                                                                                         \
        f32x4 ad[NIT];                                                                               \
        _Pragma("unroll") for (int i = 0; i < NIT; ++i) {                                            \
            CB_EPI_OFFS(i, TID, STRIDE)                                                              \
            ad[i] = *reinterpret_cast<const f32x4*>(abase + (long)co_ * a_sC + opix_);               \
        }                                                                                            \
        if (add_kind == 1) { CB_EPI_FINISH(ad[i][j], 0.f, 0.f, TID, STRIDE, BIAS) }                  \
        else if (add_kind == 2) { CB_EPI_FINISH(0.f, ad[i][j], 0.f, TID, STRIDE, BIAS) }             \
        else { CB_EPI_FINISH(0.f, 0.f, ad[i][j], TID, STRIDE, BIAS) }                                \
    }

// ---- the packed-output (P8) epilogue of a staged pass -----------------------------------------------------------------------
// A thread takes one pixel x 8 output channels of the staged [pixel][36] block, applies the epilogue, splits to hi / lo
// (split8, common.h) and writes two 16-byte units (lanes = consecutive pixels: coalesced).  Bias from LDS; with a
// pre-activation image its values for all items are fetched first, WITHOUT one the code path holds no vector-memory load at
// all (see the fp32 epilogue above).
// In scope: stage, p, m, n, n0, tx, ty, TW, TH, NPIX, NI8 ((pixel, 8 channels) items per thread), and uint4* y4 = p.y,
// gout = groups of 8 output channels, hw_out = Hout Wout.
#define CB_P8_ITEM(i, TID, OK, OPIX)                                                            \
    const int item_ = TID + 512 * (i);                                                         \
    const int gq_ = item_ / NPIX, px_ = item_ - gq_ * NPIX;                                    \
    const int co0_ = n0 + m * 32 + gq_ * 8;                                                    \
    const int prow_ = px_ / TW, pcol_ = px_ - prow_ * TW;                                      \
    [[maybe_unused]] const int vy_ = ty * TH + prow_, vx_ = tx * TW + pcol_;                   \
    [[maybe_unused]] const bool ok_ = OK;                                                      \
    const long opix_ = OPIX;
#define CB_P8_FINISH(PRE, TID, OK, OPIX, BIAS)                                                 \
_Pragma("unroll") for (int i = 0; i < NI8; ++i) {                                              \
    CB_P8_ITEM(i, TID, OK, OPIX)                                                               \
    if (ok_) {                                                                                 \
        float v[8];                                                                            \
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(stage + px_ * 36 + gq_ * 8);          \
        const f32x4 s1 = *reinterpret_cast<const f32x4*>(stage + px_ * 36 + gq_ * 8 + 4);      \
        _Pragma("unroll") for (int c = 0; c < 8; ++c) {                                        \
            float t = c < 4 ? s0[c] : s1[c - 4];                                               \
            t += (PRE);                                                                        \
            t += BIAS;                                                                         \
            if (p.act == CCVS_ACT_LRELU) t = lrelu01(t);                                       \
            v[c] = t * p.out_scale;                                                            \
        }                                                                                      \
        uint4 hi, lo;                                                                          \
        split8(v, hi, lo);                                                                     \
        uint4* dst = y4 + ((long)n * gout + (co0_ >> 3)) * 2 * hw_out + opix_;                 \
        cb_store16(dst, hi);                                                                   \
        cb_store16(dst + hw_out, lo);                                                          \
    }                                                                                          \
}
#define CB_EPI_P8(TID, OK, OPIX, CLAMP, BIAS)                                                  \
    if (p.pre) {                                                                               \
        float pv[NI8][8];                                                                      \
        const float* pb = p.pre + (long)(n / p.pre_div) * p.pre_sN;                            \
        _Pragma("unroll") for (int i = 0; i < NI8; ++i) {                                      \
            CB_P8_ITEM(i, TID, OK, OPIX)                                                       \
            _Pragma("unroll") for (int c = 0; c < 8; ++c) pv[i][c] = pb[(long)CLAMP(co0_ + c) * p.pre_sC + opix_]; \
        }                                                                                      \
        CB_P8_FINISH(pv[i][c], TID, OK, OPIX, BIAS)                                            \
    } else {                                                                                   \
        CB_P8_FINISH(0.f, TID, OK, OPIX, BIAS)                                                 \
    }
