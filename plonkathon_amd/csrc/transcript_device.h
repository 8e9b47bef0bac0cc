// transcript_device.h — the Fiat-Shamir transcript on the device (transcript.py:77-123 + merlin), shared by the prover
// (transcript_kernel) and the batch verifier (verify_scalars_kernel): the cooperative sponge, and the ONE schedule of labels
// and draws (tc_round).  32 lanes per proof, two proofs per
// 64-lane workgroup.  Lane i < 25 keeps Keccak lane st[i] in registers; a permutation round exchanges
// lanes through LDS (two barriers per round) instead of one thread grinding through all 25 lanes, the
// STROBE byte operations become "the lane that owns byte idx xors it", and the 255-byte challenge is
// reduced mod r by eight lanes in parallel.  Same byte stream as csrc/transcript.h (the host C-ABI
// transcript), which the tests pin against the merlin test vector and the golden proof.
// Control flow depends only on message lengths, which are the same for every proof, so the barriers
// are uniform.
#pragma once
#include "transcript.h"

#define TC_LANES 32
struct TcShared {
    uint64_t buf[2][25];
    uint8_t msg[256];
    Fr part[8];
};
struct TcState {
    uint64_t w;  // st[lane] for lane < 25
    uint32_t pos, pos_begin;
};

PLONK_DEV TcState tc_load(const MerlinState& m, unsigned lane) {
    TcState t;
    t.w = lane < 25 ? m.st[lane] : 0;
    t.pos = m.pos;
    t.pos_begin = m.pos_begin;
    return t;
}
PLONK_DEV void tc_store(const TcState& t, unsigned lane, MerlinState& m) {
    if (lane < 25) m.st[lane] = t.w;
    if (lane == 0) {
        m.pos = t.pos;
        m.pos_begin = t.pos_begin;
    }
}

// c[j] = 2^(256 j) R^2 mod r: one Montgomery multiplication maps a 256-bit chunk to chunk * 2^(256 j) in Montgomery form (tc_draw)
struct ChallengeConsts { Fr c[8]; };
static inline ChallengeConsts challenge_consts() {
    ChallengeConsts cc;
    Fr t = fp_zero<FrParams>();
    t.v[4] = 1;  // 2^128
    t = fp_to_mont(t);
    const Fr two256 = fp_mul(t, t);
    for (int i = 0; i < 8; i++) cc.c[0].v[i] = FrParams::r2(i);
    for (int j = 1; j < 8; j++) cc.c[j] = fp_mul(cc.c[j - 1], two256);
    return cc;
}

PLONK_DEV void tc_keccak(TcState& t, TcShared& sh, unsigned lane) {
    constexpr unsigned rot[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
    const bool act = lane < 25;
    const unsigned i = act ? lane : 24, x = i % 5, y = i / 5;
    const unsigned r = rot[i], dst = y + 5 * ((2 * x + 3 * y) % 5);
    const unsigned ca = (x + 4) % 5, cb = (x + 1) % 5, n1 = (x + 1) % 5 + 5 * y, n2 = (x + 2) % 5 + 5 * y;
    uint64_t a = t.w;
    for (int round = 0; round < 24; round++) {
        if (act) sh.buf[0][i] = a;
        __syncthreads();
        uint64_t c0 = 0, c1 = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            c0 ^= sh.buf[0][ca + 5 * k];
            c1 ^= sh.buf[0][cb + 5 * k];
        }
        a ^= c0 ^ keccak_rotl(c1, 1);
        if (act) sh.buf[1][dst] = keccak_rotl(a, r);
        __syncthreads();
        a = sh.buf[1][i] ^ (~sh.buf[1][n1] & sh.buf[1][n2]);
        if (i == 0) a ^= keccak_rc(round);
    }
    t.w = a;
}

PLONK_DEV void tc_xor_byte(TcState& t, unsigned lane, unsigned idx, uint8_t b) {
    if (lane == (idx >> 3)) t.w ^= (uint64_t)b << (8 * (idx & 7));
}
PLONK_DEV void tc_run_f(TcState& t, TcShared& sh, unsigned lane) {
    tc_xor_byte(t, lane, t.pos, (uint8_t)t.pos_begin);
    tc_xor_byte(t, lane, t.pos + 1, 0x04);
    tc_xor_byte(t, lane, STROBE_R + 1, 0x80);
    tc_keccak(t, sh, lane);
    t.pos = 0;
    t.pos_begin = 0;
}
PLONK_DEV void tc_absorb_byte(TcState& t, TcShared& sh, unsigned lane, uint8_t b) {
    tc_xor_byte(t, lane, t.pos, b);
    if (++t.pos == STROBE_R) tc_run_f(t, sh, lane);
}
// data: constant / global / LDS bytes readable by every lane of the group
PLONK_DEV void tc_absorb(TcState& t, TcShared& sh, unsigned lane, const uint8_t* data, unsigned n) {
    while (n) {
        const unsigned take = n < STROBE_R - t.pos ? n : STROBE_R - t.pos;
#pragma unroll
        for (unsigned j = 0; j < 8; j++) {
            const unsigned idx = 8 * lane + j;
            if (idx >= t.pos && idx < t.pos + take) t.w ^= (uint64_t)data[idx - t.pos] << (8 * j);
        }
        t.pos += take;
        data += take;
        n -= take;
        if (t.pos == STROBE_R) tc_run_f(t, sh, lane);
    }
}
PLONK_DEV void tc_squeeze(TcState& t, TcShared& sh, unsigned lane, uint8_t* out, unsigned n) {
    while (n) {
        const unsigned take = n < STROBE_R - t.pos ? n : STROBE_R - t.pos;
#pragma unroll
        for (unsigned j = 0; j < 8; j++) {
            const unsigned idx = 8 * lane + j;
            if (idx >= t.pos && idx < t.pos + take) {
                out[idx - t.pos] = (uint8_t)(t.w >> (8 * j));
                t.w &= ~((uint64_t)0xff << (8 * j));
            }
        }
        t.pos += take;
        out += take;
        n -= take;
        if (t.pos == STROBE_R) tc_run_f(t, sh, lane);
    }
}
PLONK_DEV void tc_begin_op(TcState& t, TcShared& sh, unsigned lane, uint32_t flags) {
    const uint8_t h0 = (uint8_t)t.pos_begin;
    t.pos_begin = t.pos + 1;
    tc_absorb_byte(t, sh, lane, h0);
    tc_absorb_byte(t, sh, lane, (uint8_t)flags);
    if ((flags & (STROBE_FLAG_C | STROBE_FLAG_K)) && t.pos != 0) tc_run_f(t, sh, lane);
}
// meta-AD of label || u32le(len): the framing merlin puts in front of every message and challenge
PLONK_DEV void tc_frame(TcState& t, TcShared& sh, unsigned lane, const char* label, unsigned llen, unsigned len) {
    tc_begin_op(t, sh, lane, STROBE_FLAG_M | STROBE_FLAG_A);
    tc_absorb(t, sh, lane, (const uint8_t*)label, llen);
    for (int k = 0; k < 4; k++) tc_absorb_byte(t, sh, lane, (uint8_t)(len >> (8 * k)));
}
PLONK_DEV void tc_append_message(TcState& t, TcShared& sh, unsigned lane, const char* label, unsigned llen,
                                 const uint8_t* msg, unsigned mlen) {
    tc_frame(t, sh, lane, label, llen, mlen);
    tc_begin_op(t, sh, lane, STROBE_FLAG_A);
    tc_absorb(t, sh, lane, msg, mlen);
}

// challenge_bytes(label, 255) read as a big-endian integer mod r (the reference's wide reduction: no bias), zero included and nothing
// re-appended.  The 255 bytes stay in sh.msg; every lane of the group gets the value (Montgomery form).  (tc_draw below repeats
// these lines, and round 0 of tc_round those of tc_open, on purpose: calling the shared halves from there changes the code of
// transcript_kernel and verify_scalars_kernel — profiles/blinding_kernel_compare.txt.)
PLONK_DEV Fr tc_challenge_wide(TcState& t, TcShared& sh, unsigned lane, const ChallengeConsts& cc, const char* label, unsigned llen) {
    tc_frame(t, sh, lane, label, llen, 255);
    tc_begin_op(t, sh, lane, STROBE_FLAG_I | STROBE_FLAG_A | STROBE_FLAG_C);
    __syncthreads();  // earlier readers of sh.msg are done
    tc_squeeze(t, sh, lane, sh.msg, 255);
    __syncthreads();
    if (lane < 8) {  // chunk 0 = the leading 31 bytes, chunk c >= 1 = the next 32; weight 2^(256 (7 - c))
        const unsigned take = lane ? 32 : 31, off = lane ? 31 + 32 * (lane - 1) : 0;
        Fr chunk;  // little-endian limbs of the big-endian chunk
#pragma unroll
        for (unsigned l = 0; l < 8; l++) {
            uint32_t wv = 0;
#pragma unroll
            for (unsigned k = 0; k < 4; k++) {
                const unsigned sig = 4 * l + k;  // byte significance within the chunk
                if (sig < take) wv |= (uint32_t)sh.msg[off + take - 1 - sig] << (8 * k);
            }
            chunk.v[l] = wv;
        }
        sh.part[lane] = fp_mul(chunk, cc.c[7 - lane]);
    }
    __syncthreads();
    Fr f = sh.part[0];
    for (int k = 1; k < 8; k++) f = fp_add(f, sh.part[k]);
    return f;
}

// transcript.py:69-75: 255 PRF bytes -> big-endian integer mod r (retry on zero) -> re-appended.  Returns the
// challenge (Montgomery form) in every lane of the group.
PLONK_DEV Fr tc_draw(TcState& t, TcShared& sh, unsigned lane, const ChallengeConsts& cc, const char* label, unsigned llen) {
    for (;;) {
        tc_frame(t, sh, lane, label, llen, 255);
        tc_begin_op(t, sh, lane, STROBE_FLAG_I | STROBE_FLAG_A | STROBE_FLAG_C);
        __syncthreads();  // earlier readers of sh.msg are done
        tc_squeeze(t, sh, lane, sh.msg, 255);
        __syncthreads();
        if (lane < 8) {  // chunk 0 = the leading 31 bytes, chunk c >= 1 = the next 32; weight 2^(256 (7 - c))
            const unsigned take = lane ? 32 : 31, off = lane ? 31 + 32 * (lane - 1) : 0;
            Fr chunk;  // little-endian limbs of the big-endian chunk
#pragma unroll
            for (unsigned l = 0; l < 8; l++) {
                uint32_t wv = 0;
#pragma unroll
                for (unsigned k = 0; k < 4; k++) {
                    const unsigned sig = 4 * l + k;  // byte significance within the chunk
                    if (sig < take) wv |= (uint32_t)sh.msg[off + take - 1 - sig] << (8 * k);
                }
                chunk.v[l] = wv;
            }
            sh.part[lane] = fp_mul(chunk, cc.c[7 - lane]);
        }
        __syncthreads();
        Fr f = sh.part[0];
        for (int k = 1; k < 8; k++) f = fp_add(f, sh.part[k]);
        if (!fp_is_zero(f)) {
            tc_append_message(t, sh, lane, label, llen, sh.msg, 255);
            return f;
        }
    }
}

// MerlinTranscript(label): the STROBE-128 state under "Merlin v1.0", then the domain separator
PLONK_DEV void tc_open(TcState& t, TcShared& sh, unsigned lane, const char* label, unsigned llen) {
    const uint8_t init[18] = {1, STROBE_R + 2, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
    t.w = 0;
    for (unsigned j = 0; j < 8; j++)
        if (8 * lane + j < 18) t.w |= (uint64_t)init[8 * lane + j] << (8 * j);
    tc_keccak(t, sh, lane);
    t.pos = 0;
    t.pos_begin = 0;
    tc_begin_op(t, sh, lane, STROBE_FLAG_M | STROBE_FLAG_A);
    tc_absorb(t, sh, lane, (const uint8_t*)"Merlin v1.0", 11);
    tc_append_message(t, sh, lane, "dom-sep", 7, (const uint8_t*)label, llen);
}

// The schedule.  Round 0 opens Transcript(b"plonk") (prover.py:53); rounds 1-4 are the prover's (transcript.py:77-116), round 5
// is the one only a verifier reaches (TESTING_verifier:276-277).  The caller has staged the round's messages in sh.msg, 32
// big-endian bytes each — a commitment is x then y (transcript.py:62-67) — behind a barrier; the round appends them under their
// labels and draws its challenges into c0 (and c1, rounds 1 and 2).
PLONK_DEV void tc_round(TcState& t, TcShared& sh, unsigned lane, const ChallengeConsts& cc, int round, Fr& c0, Fr& c1) {
    const auto point = [&](int k, const char* label, unsigned llen) {
        tc_append_message(t, sh, lane, label, llen, sh.msg + 64 * k, 32);
        tc_append_message(t, sh, lane, label, llen, sh.msg + 64 * k + 32, 32);
    };
    if (round == 0) {
        const uint8_t init[18] = {1, STROBE_R + 2, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
        t.w = 0;
        for (unsigned j = 0; j < 8; j++)
            if (8 * lane + j < 18) t.w |= (uint64_t)init[8 * lane + j] << (8 * j);
        tc_keccak(t, sh, lane);
        t.pos = 0;
        t.pos_begin = 0;
        tc_begin_op(t, sh, lane, STROBE_FLAG_M | STROBE_FLAG_A);
        tc_absorb(t, sh, lane, (const uint8_t*)"Merlin v1.0", 11);
        tc_append_message(t, sh, lane, "dom-sep", 7, (const uint8_t*)"plonk", 5);
    } else if (round == 1) {
        point(0, "a_1", 3);
        point(1, "b_1", 3);
        point(2, "c_1", 3);
        c0 = tc_draw(t, sh, lane, cc, "beta", 4);
        c1 = tc_draw(t, sh, lane, cc, "gamma", 5);
    } else if (round == 2) {
        point(0, "z_1", 3);
        c0 = tc_draw(t, sh, lane, cc, "alpha", 5);
        c1 = tc_draw(t, sh, lane, cc, "fft_cofactor", 12);
    } else if (round == 3) {
        point(0, "t_lo_1", 6);
        point(1, "t_mid_1", 7);
        point(2, "t_hi_1", 6);
        c0 = tc_draw(t, sh, lane, cc, "zeta", 4);
    } else if (round == 4) {
        tc_append_message(t, sh, lane, "a_eval", 6, sh.msg, 32);
        tc_append_message(t, sh, lane, "b_eval", 6, sh.msg + 32, 32);
        tc_append_message(t, sh, lane, "c_eval", 6, sh.msg + 64, 32);
        tc_append_message(t, sh, lane, "s1_eval", 7, sh.msg + 96, 32);
        tc_append_message(t, sh, lane, "s2_eval", 7, sh.msg + 128, 32);
        tc_append_message(t, sh, lane, "z_shifted_eval", 14, sh.msg + 160, 32);
        c0 = tc_draw(t, sh, lane, cc, "v", 1);
    } else if (round == 5) {
        point(0, "W_z_1", 5);
        point(1, "W_zw_1", 6);
        c0 = tc_draw(t, sh, lane, cc, "u", 1);
    }
}
