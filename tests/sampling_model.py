# -*- coding: utf-8 -*-
"""numpy fp64 model of the device sampler (csrc/la_sample.hip, include/lookahead_hip.h "sampling on the device").

Integer parts (Philox4x32-10, the 16-bit keys, the top-k threshold) are exact; the float parts (temperature, softmax mass, Gumbel
score) are computed in fp64 and compared with the kernel's fp32 through stated margins (tests/test_gpu_sampling.py)."""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(ctr, key, rounds=10):
    """Philox4x32-`rounds` (Salmon et al., SC'11).  ctr: uint32 [..., 4], key: two uint32 (scalars or [...]) -> uint32 [..., 4]."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0 = np.asarray(key[0]).astype(np.uint64) & _M32
    k1 = np.asarray(key[1]).astype(np.uint64) & _M32
    for _ in range(rounds):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack(c, axis=-1).astype(np.uint32)


def sample_bits(seed, stream, position, vocab):
    """uint32 [vocab]: token v's Philox word — counter (v >> 2, position, stream, 0), key (seed lo, seed hi), output word v & 3.
    `position` = the index in the unpadded sequence of the token being chosen (= RoPE position of the row + 1)."""
    quads = (vocab + 3) // 4
    ctr = np.zeros((quads, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(quads, dtype=np.uint32)
    ctr[:, 1] = np.uint32(position & 0xFFFFFFFF)
    ctr[:, 2] = np.uint32(stream & 0xFFFFFFFF)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:vocab]


def uniform_of(bits):
    """u = (top 23 bits + 0.5) * 2^-23: exact in fp32, never 0 or 1"""
    return ((bits >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_of(bits):
    return -np.log(-np.log(uniform_of(bits)))


# ---- 16-bit storage <-> value <-> key ---------------------------------------------------------------------------------------------
def bits_to_f64(bits, dtype):
    """uint16 storage bits -> float64 values; dtype 'bf16' or 'fp16'"""
    bits = np.asarray(bits, dtype=np.uint16)
    if dtype == 'fp16':
        return bits.view(np.float16).astype(np.float64)
    with np.errstate(invalid='ignore'):                       # signalling NaN patterns
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def f32_to_bits(x, dtype):
    """float32 -> storage bits, round to nearest even (what torch and the kernels do)"""
    x = np.asarray(x, dtype=np.float32)
    if dtype == 'fp16':
        with np.errstate(over='ignore'):
            return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, (u | np.uint32(0x400000)) >> np.uint32(16), r).astype(np.uint16)


def keys_of(bits, dtype):
    """monotone 16-bit key: unsigned order == value order, -0 folded into +0, NaN -> 0 (never kept)"""
    u = np.asarray(bits, dtype=np.uint16).astype(np.uint32)
    mag = u & 0x7FFF
    inf = 0x7C00 if dtype == 'fp16' else 0x7F80
    u = np.where(mag == 0, 0, u)
    key = np.where(u & 0x8000, ~u & 0xFFFF, u | 0x8000)
    return np.where(mag > inf, 0, key).astype(np.uint32)


def key_to_f64(key, dtype):
    key = np.asarray(key, dtype=np.uint32)
    bits = np.where(key & 0x8000, key & 0x7FFF, ~key & 0xFFFF).astype(np.uint16)
    return bits_to_f64(bits, dtype)


def penalised_bits(bits, dtype, members, penalty):
    """the repetition penalty on the members of the context (boolean [vocab]): fp32 multiply / divide, rounded to the storage type"""
    v = bits_to_f64(bits, dtype).astype(np.float32)
    p = np.float32(penalty)
    with np.errstate(over='ignore', invalid='ignore'):
        pv = np.where(v < 0, v * p, v / p).astype(np.float32)
    return np.where(members, f32_to_bits(pv, dtype), np.asarray(bits, dtype=np.uint16)).astype(np.uint16)


# ---- the filter ---------------------------------------------------------------------------------------------------------------------
def topk_key(keys, top_k):
    """the key of the k-th largest value; 0 = off (top_k <= 0, >= vocab, or more than the row has non-NaN values)"""
    vocab = len(keys)
    if top_k <= 0 or top_k >= vocab:
        return 0
    valid = np.sort(keys[keys > 0])[::-1]
    return int(valid[top_k - 1]) if top_k <= len(valid) else 0


def masses(keys, dtype, temperature, floor_key):
    """fp64 softmax numerators exp(z - z_max) of the survivors (key >= max(floor_key, 1)), 0 elsewhere; z = x / float32(temperature)"""
    T = float(np.float32(temperature))
    surv = keys >= max(int(floor_key), 1)
    z = key_to_f64(keys, dtype) / T
    zmax = z[keys > 0].max()
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.where(surv, np.exp(np.where(surv, z - zmax, -np.inf)), 0.0)
    m[keys == keys.max()] = 1.0 if keys.max() >= max(int(floor_key), 1) else 0.0
    return m, surv


def mass_above(keys, m, key, strict=True):
    """normalised mass of the survivors with key > `key` (strict) or >= `key`"""
    sel = keys > key if strict else keys >= key
    return float(m[sel].sum() / m.sum())


def topp_key(keys, m, top_p):
    """the lowest key kept by top-p: keep v iff the mass of survivors with a strictly greater value is < top_p.  0 = off (top_p >= 1)."""
    if top_p >= 1.0:
        return 0
    present = np.unique(keys[m > 0])[::-1]                     # descending
    tot = np.array([m[keys == k].sum() for k in present]) / m.sum()
    above = np.concatenate([[0.0], np.cumsum(tot)[:-1]])       # mass strictly above each present key
    kept = present[above < max(top_p, 0.0)]
    return int(kept.min()) if len(kept) else int(present[0])


def kept_mask(keys, k_key, p_key):
    return keys >= max(int(k_key), int(p_key), 1)


def filter_row(bits, dtype, temperature, top_k, top_p):
    """-> (top-k key, top-p key, kept mask) of one row of storage bits"""
    keys = keys_of(bits, dtype)
    kk = topk_key(keys, top_k)
    m, _ = masses(keys, dtype, temperature, kk)
    kp = topp_key(keys, m, top_p)
    return kk, kp, kept_mask(keys, kk, kp)


# ---- the draw -----------------------------------------------------------------------------------------------------------------------
def scores_of(bits, dtype, temperature, rng_bits):
    """fp64 z + g of every token"""
    z = bits_to_f64(bits, dtype) / float(np.float32(temperature))
    return z + gumbel_of(rng_bits)


def pick(bits, dtype, temperature, kept, rng_bits):
    """-> (token, gap): the fp64 argmax of z + g over the kept set (lowest index among equals) and the top-1 / top-2 gap
    (inf when one token is kept)"""
    with np.errstate(invalid='ignore'):
        s = np.where(kept, scores_of(bits, dtype, temperature, rng_bits), -np.inf)
    s = np.where(np.isnan(s), -np.inf, s)
    tok = int(np.argmax(s))
    if kept.sum() < 2:
        return tok, np.inf
    top2 = np.partition(s, -2)[-2:]
    return tok, float(top2[1] - top2[0])


def sample_row(bits, dtype, position, stream, seed, temperature, top_k, top_p, members=None, penalty=None):
    """the whole sampler on one row -> token"""
    if members is not None:
        bits = penalised_bits(bits, dtype, members, penalty)
    _, _, kept = filter_row(bits, dtype, temperature, top_k, top_p)
    return pick(bits, dtype, temperature, kept, sample_bits(seed, stream, position, len(bits)))[0]


def torch_bits(t):
    """a torch bf16 / fp16 tensor -> (uint16 numpy bits, dtype name)"""
    import torch
    name = 'fp16' if t.dtype == torch.float16 else 'bf16'
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), name
