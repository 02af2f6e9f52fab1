"""numpy restatement of ggml's CPU dequantize_row_* for the decode-only block types (Q4_0, Q4_1, Q5_0, Q5_1, Q2_K,
Q3_K, Q5_K, IQ4_NL), written from the block structs (ggml-common.h) and the dequantize / quantize functions of ggml's
Metal source, independent of the library's C++.  All arithmetic in float32: every product below is an fp16 scale times
a small integer (exact), so each value rounds at most once, as in ggml's C.

Blocks are uint8 arrays [rows][nb][block bytes]; results are float32 [rows][nb * block values]."""
import numpy as np

BLOCK = {"q4_0": (32, 18), "q4_1": (32, 20), "q5_0": (32, 22), "q5_1": (32, 24), "q8_0": (32, 34), "q2_k": (256, 84),
         "q3_k": (256, 110), "q4_k": (256, 144), "q5_k": (256, 176), "q6_k": (256, 210), "iq4_nl": (32, 18)}
NEW_TYPES = ("q4_0", "q4_1", "q5_0", "q5_1", "q2_k", "q3_k", "q5_k", "iq4_nl")
KVALUES_IQ4NL = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], dtype=np.float32)
F = np.float32


def _f16(b, off):
    """fp16 field at byte offset off of every block -> float32 [rows][nb][1]"""
    return np.ascontiguousarray(b[..., off:off + 2]).view("<f2").astype(F)


def _nibbles(qs):
    """[..., 16] bytes -> [..., 32]: low nibbles first (values 0..15), then high nibbles (16..31)"""
    return np.concatenate([qs & 0xF, qs >> 4], axis=-1).astype(np.int32)


def _qh_bits(qh):
    """[..., 4] bytes (little-endian u32) -> [..., 32] bits, bit v = fifth bit of value v"""
    return np.unpackbits(qh, axis=-1, bitorder="little").astype(np.int32)


def dequant(blocks: np.ndarray, qtype: str) -> np.ndarray:
    b = np.ascontiguousarray(blocks, dtype=np.uint8)
    rows, nb, bb = b.shape
    assert bb == BLOCK[qtype][1], (qtype, bb)
    if qtype == "q4_0":      # {d, qs[16]}: (q - 8) * d
        y = (_nibbles(b[..., 2:18]) - 8).astype(F) * _f16(b, 0)
    elif qtype == "q4_1":    # {d, m, qs[16]}: q * d + m
        y = _nibbles(b[..., 4:20]).astype(F) * _f16(b, 0) + _f16(b, 2)
    elif qtype == "q5_0":    # {d, qh[4], qs[16]}: (q5 - 16) * d
        q = _nibbles(b[..., 6:22]) | (_qh_bits(b[..., 2:6]) << 4)
        y = (q - 16).astype(F) * _f16(b, 0)
    elif qtype == "q5_1":    # {d, m, qh[4], qs[16]}: q5 * d + m
        q = _nibbles(b[..., 8:24]) | (_qh_bits(b[..., 4:8]) << 4)
        y = q.astype(F) * _f16(b, 0) + _f16(b, 2)
    elif qtype == "iq4_nl":  # {d, qs[16]}: d * kvalues[q]
        y = _f16(b, 0) * KVALUES_IQ4NL[_nibbles(b[..., 2:18])]
    elif qtype == "q8_0":    # {d, qs[32] int8}
        y = b[..., 2:34].view(np.int8).astype(F) * _f16(b, 0)
    elif qtype == "q2_k":    # {scales[16], qs[64], d, dmin}: per 16 values dl * q2 - ml
        sc = b[..., 0:16].astype(np.int32)
        dl = _f16(b, 80) * (sc & 0xF).astype(F)      # [rows][nb][16]
        ml = _f16(b, 82) * (sc >> 4).astype(F)
        qs = b[..., 16:80].reshape(rows, nb, 2, 1, 32).astype(np.int32)  # [half n][.][l]
        shifts = np.arange(4, dtype=np.int32).reshape(1, 1, 1, 4, 1) * 2
        q = ((qs >> shifts) & 3).reshape(rows, nb, 16, 16)               # value 128n + 32j + l -> group 8n + 2j + l/16
        y = (dl[..., None] * q.astype(F) - ml[..., None]).reshape(rows, nb, 256)
    elif qtype == "q3_k":    # {hmask[32], qs[64], scales[12], d}: dl * (q2 - (hmask bit ? 0 : 4)), dl = d * (sc6 - 32)
        s = b[..., 96:108].astype(np.int32)
        k = np.arange(16)
        lo = np.where(k < 8, s[..., k % 8] & 0xF, s[..., k % 8] >> 4)
        hi = (s[..., 8 + (k & 3)] >> (2 * (k >> 2))) & 3
        dl = _f16(b, 108) * ((lo | (hi << 4)) - 32).astype(F)            # [rows][nb][16]
        qs = b[..., 32:96].reshape(rows, nb, 2, 1, 32).astype(np.int32)
        shifts = np.arange(4, dtype=np.int32).reshape(1, 1, 1, 4, 1) * 2
        q = (qs >> shifts) & 3                                           # [rows][nb][n][j][l]
        hm = b[..., 0:32].reshape(rows, nb, 1, 1, 32).astype(np.int32)
        bit = (np.arange(2).reshape(1, 1, 2, 1, 1) * 4 + np.arange(4).reshape(1, 1, 1, 4, 1))
        q = q - np.where((hm >> bit) & 1, 0, 4)
        y = (dl[..., None] * q.reshape(rows, nb, 16, 16).astype(F)).reshape(rows, nb, 256)
    elif qtype in ("q4_k", "q5_k"):  # {d, dmin, scales[12], [qh[32],] qs[128]}: per 32 values d1 * q - m1
        s = b[..., 4:16].astype(np.int32)
        sc = np.empty((rows, nb, 8), dtype=np.int32)
        mn = np.empty((rows, nb, 8), dtype=np.int32)
        for i in range(8):   # get_scale_min_k4
            if i < 4:
                sc[..., i] = s[..., i] & 63
                mn[..., i] = s[..., i + 4] & 63
            else:
                sc[..., i] = (s[..., i + 4] & 0xF) | ((s[..., i - 4] >> 6) << 4)
                mn[..., i] = (s[..., i + 4] >> 4) | ((s[..., i] >> 6) << 4)
        d1 = _f16(b, 0) * sc.astype(F)
        m1 = _f16(b, 2) * mn.astype(F)
        qo = 16 if qtype == "q4_k" else 48
        qs = b[..., qo:qo + 128].reshape(rows, nb, 4, 32).astype(np.int32)
        q = np.stack([qs & 0xF, qs >> 4], axis=3).reshape(rows, nb, 8, 32)  # sub-block 2g: low nibbles, 2g+1: high
        if qtype == "q5_k":
            qh = b[..., 16:48].reshape(rows, nb, 1, 32).astype(np.int32)
            q = q + (((qh >> np.arange(8).reshape(1, 1, 8, 1)) & 1) << 4)
        y = (d1[..., None] * q.astype(F) - m1[..., None]).reshape(rows, nb, 256)
    elif qtype == "q6_k":    # {ql[128], qh[64], scales[16] int8, d}
        ql = b[..., 0:128].reshape(rows, nb, 2, 2, 32).astype(np.int32)     # [half][+0 / +32][l]
        qh = b[..., 128:192].reshape(rows, nb, 2, 1, 32).astype(np.int32)
        lo = np.concatenate([ql & 0xF, ql >> 4], axis=3)                    # quarters 0, 1 (low), 2, 3 (high)
        h2 = (qh >> (np.arange(4).reshape(1, 1, 1, 4, 1) * 2)) & 3
        q = (lo | (h2 << 4)) - 32
        ds = _f16(b, 208) * b[..., 192:208].view(np.int8).astype(F)         # [rows][nb][16]
        y = (ds[..., None] * q.reshape(rows, nb, 16, 16).astype(F)).reshape(rows, nb, 256)
    else:
        raise ValueError(qtype)
    return np.ascontiguousarray(y.reshape(rows, -1), dtype=F)


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """rne_bf16 of finite float32 values, as uint16 words"""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---- ggml's short encoders (quantize_q4_0 / q4_1 / q5_0 / q5_1 / iq4_nl of the Metal source), for the round-trip check
def _amax_signed(x):
    i = np.argmax(np.abs(x), axis=-1)
    return np.take_along_axis(x, i[..., None], axis=-1)


def _pack_nibbles(q):
    return (q[..., :16] | (q[..., 16:] << 4)).astype(np.uint8)


def _pack_qh(q):
    return np.packbits(((q >> 4) & 1).astype(np.uint8), axis=-1, bitorder="little")


def quantize(x: np.ndarray, qtype: str) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=F)
    rows, cols = x.shape
    xb = x.reshape(rows, cols // 32, 32)
    out = np.zeros((rows, cols // 32, BLOCK[qtype][1]), dtype=np.uint8)

    def put16(off, v):
        out[..., off:off + 2] = v.astype("<f2").view(np.uint8).reshape(rows, -1, 2)

    if qtype in ("q4_0", "q5_0", "iq4_nl"):
        mx = _amax_signed(xb)
        div = {"q4_0": F(-8), "q5_0": F(-16), "iq4_nl": KVALUES_IQ4NL[0]}[qtype]
        d = (mx / div).astype(F)
        idv = np.where(d != 0, F(1) / np.where(d != 0, d, F(1)), F(0)).astype(F)
        t = xb * idv
        if qtype == "q4_0":
            q = np.minimum(15, (t + F(8.5)).astype(np.int8)).astype(np.int32)
            put16(0, d)
            out[..., 2:18] = _pack_nibbles(q)
        elif qtype == "q5_0":
            q = np.minimum(31, (t + F(16.5)).astype(np.int8)).astype(np.int32)
            put16(0, d)
            out[..., 2:6] = _pack_qh(q)
            out[..., 6:22] = _pack_nibbles(q & 0xF)
        else:  # best_index_int8: the nearest table value
            q = np.argmin(np.abs(t[..., None] - KVALUES_IQ4NL), axis=-1).astype(np.int32)
            put16(0, d)  # (the Metal encoder then refits d by least squares; the plain d is a valid encoding too)
            out[..., 2:18] = _pack_nibbles(q)
    else:
        mn, mx = xb.min(-1, keepdims=True), xb.max(-1, keepdims=True)
        levels = F(15) if qtype == "q4_1" else F(31)
        d = ((mx - mn) / levels).astype(F)
        idv = np.where(d != 0, F(1) / np.where(d != 0, d, F(1)), F(0)).astype(F)
        q = np.minimum(int(levels), ((xb - mn) * idv + F(0.5)).astype(np.int32))
        put16(0, d)
        put16(2, mn)
        if qtype == "q4_1":
            out[..., 4:20] = _pack_nibbles(q)
        else:
            out[..., 4:8] = _pack_qh(q)
            out[..., 8:24] = _pack_nibbles(q & 0xF)
    return out
