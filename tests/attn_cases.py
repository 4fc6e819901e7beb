"""Case builders and references for the split-key cross attention (csrc/attn.hip); numpy and torch-CPU only.

Three things live here:

* selector cases whose outputs and gradients are known in closed form (`single_case`, `tie_case`, `nomatch_case`): queries
  and selected keys are 4 x rows of the 16 x 16 Sylvester Hadamard matrix, every other key is zero, so with scale 1/4 a logit is
  64 on a match and 0 elsewhere; V and dO are small integers, so every product and sum is exact in fp32;
* `reference`: the same attention in fp64 with the kernels' rounding points (P, O, dS to bf16) -- what the closed forms are
  checked against on the CPU, and what `lse` is compared with on the GPU;
* `keep_mask`: the dropout hash of the kernels restated in numpy uint32 arithmetic, with the step-counter seed mixing.

Closed forms, with P = softmax weights, A = P (x keep / (1 - p)), dA = dO V^T, D = rowsum(dO o O), scale = 1/4:
  O = bf16(bf16(A) V),  dV = bf16(bf16(A)^T dO),  dS = bf16(P o (dA - D) scale),  dQ = bf16(dS K),  dK = bf16(dS^T Q).
One selected key: P = 1 there (the other keys weigh exp(-64) each, < 1e-23 in all), dA = D there, so dS = 0.
Two selected keys a, b with the same code: P = 1/2 at both, O = (V_a + V_b) / 2, dA_a - D = dO.(V_a - V_b) / 2, hence
dS = +-dO.(V_a - V_b) / 16 (1/2 for P, 1/4 for the scale); dQ = dS_a K_a + dS_b K_b = 0 because K_a = K_b.
No match (Q = 0): every weight is 1 / Lk, rounded to bf16 BEFORE it meets V (the kernels feed bf16 weights to the second
MFMA), so O = bf16(bf16(1 / Lk) sum V): the mean of V exactly where Lk is a power of two, one weight rounding away elsewhere.

NO CANCELLATION.  The exp(-64) weights of the unselected keys do not simply vanish in the matrix core's accumulators.  Measured
on an MI355X with single v_mfma_f32_16x16x16_bf16 instructions: the adder aligns every term to the largest one, keeps one bit
below the fp32 result and floors, so a term of -2^-90 still takes that bit (2^-24 of the largest term) off the sum:
accumulator -2^-90 with products 4 and -4 gives -2^-22, not 0; with the one product 4 it gives 3.99999976; with the one product
5 it gives 5 (the bit is rounded back).  A sum that cancels INSIDE one instruction therefore keeps a residue of 2^-24 of its
largest term, and a sum that cancels across instructions keeps one where a partial sum was a power of two.  Sums that end
non-zero are unharmed: the bit is rounded away in bf16.  So at logit 64 the builders keep the sums whose closed form is zero
free of non-zero partial sums wherever the case allows (`steady`): dO has one sign per (batch, head, channel) and no zero and
V_a - V_b takes that sign, which makes every sum over queries in dV and dK monotone and non-zero, and x = dO.(V_a - V_b) is kept
off the powers of two.  What is left is dQ of the tie case, x/4 h - x/4 h by construction: where the two keys share a 16-key
tile the two halves meet in one instruction; that one is settled in the kernel (attn_bwd_kernel counts weights below e^-40
as zero), so the backward leaves no exp(-64) residue at all, while the forward still does.  With the codes x 8 (`amp=8`,
logit 256) the unselected weights underflow to exactly zero; there dO and V_a - V_b are free in sign, sums cancel through whatever partial sums they like, and every zero of
a closed form is an exact zero, dQ of the ties included.
"""
import numpy as np
import torch

KEY_COUNTS = (70, 512, 513, 1100, 1536, 2049)
QUERY_COUNTS = (1, 16, 17, 200, 256, 257, 500, 512)
# (B, H, Lq, Lk): every key count, every query count, both backward instantiations (Lq <= 256 / above), B = 2 and H = 3 thrice
PAIRS = ((1, 1, 1, 70), (1, 2, 16, 512), (2, 3, 17, 513), (1, 2, 200, 1100), (1, 1, 256, 1536), (1, 2, 257, 2049),
         (1, 1, 500, 70), (1, 2, 512, 513), (2, 3, 257, 1100), (1, 1, 512, 2049), (2, 3, 200, 2049), (1, 1, 16, 1536))
SCALE = 0.25
TINY = 1e-20  # what exp(-64) leaves behind where the closed form is zero

SEED_STEP = 0xD1B54A32D192ED03  # csrc/attn.hip eff_seed
M64 = (1 << 64) - 1


def hadamard16():
    h = np.ones((1, 1))
    for _ in range(4):
        h = np.block([[h, h], [h, -h]])
    return h


def bf16_round(x):
    """fp64 -> bf16 (round to nearest even) -> fp64."""
    return torch.as_tensor(x, dtype=torch.float64).to(torch.bfloat16).double()


def as_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def query_code(Lq, bh, ncodes=16):
    """Code of every query of (batch, head) pair bh: every query carries one, the assignment shifts from tile to tile."""
    q = np.arange(Lq)
    return (q + q // 16 + bh) % ncodes


def single_positions(Lk):
    """16 distinct key positions: lane-group, tile, wave and chunk seams, the last key, the first key of the ragged tile."""
    want = [0, 3, 4, 15, 16, 127, 128, 511, 512, Lk - 1]
    if Lk % 16:
        want.append(Lk // 16 * 16)
    want += [1023, 1024, 1535, 1536, 2047, Lk - 2, 63, 64, 1, 33, 47, 20, 9, 2, 5, 30, 50, 60]
    pos = []
    for p in want:
        if 0 <= p < Lk and p not in pos:
            pos.append(p)
    return pos[:16]


def tie_pairs(Lk):
    """Pairs of key positions that share a code: same lane group, adjacent lane groups, tiles, waves, chunks, first and last
    chunk, into the ragged tile, inside it."""
    want = [(8, 10), (3, 4), (15, 16), (127, 128), (511, 512), (40, Lk - 1), (1023, 1024), (Lk // 16 * 16 - 1, Lk // 16 * 16),
            (Lk - 4, Lk - 3), (255, 256), (130, 1030)]
    used, pairs = set(), []
    for a, b in want:
        if 0 <= a < b < Lk and a not in used and b not in used:
            pairs.append((a, b))
            used.update((a, b))
    return pairs[:16]


def _ints(rng, shape, lo, hi, nonzero=False):
    x = rng.integers(lo, hi + 1, shape)
    if nonzero:
        x = np.where(x == 0, hi, x)
    return x.astype(np.float64)


def _heads(x, H):
    """[B, L, H*16] -> [B, H, L, 16]"""
    B, L, E = x.shape
    return x.reshape(B, L, H, 16).transpose(0, 2, 1, 3)


def _unheads(x):
    B, H, L, d = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B, L, H * d)


def _pack(name, H, q, k, v, do, expect):
    return dict(name=name, H=H, q=as_bf16(_unheads(q)), k=as_bf16(_unheads(k)), v=as_bf16(_unheads(v)), do=as_bf16(_unheads(do)),
                expect={n: torch.from_numpy(_unheads(e)) for n, e in expect.items()})


def _grad_out(rng, B, H, Lq, steady):
    """dO: integers in [-8, 8]; steady: none zero and one sign per (batch, head, channel), so that no sum over queries cancels."""
    if not steady:
        return _ints(rng, (B, H, Lq, 16), -8, 8), None
    sign = rng.choice([-1.0, 1.0], (B, H, 1, 16))
    return sign * _ints(rng, (B, H, Lq, 16), 1, 8), sign[:, :, 0]


def _is_pow2(x):
    x = int(abs(x))
    return x > 0 and x & (x - 1) == 0


def single_case(B, H, Lq, Lk, seed=0, amp=4, steady=None):
    """One selected key per code.  O = V[sel]; dV[sel] = sum of dO over the queries that select it (rounded once), zero
    elsewhere; dQ = dK = 0 (dS is an exact zero at the selected key).  V has no zero entry, so O leaves no exp(-64) residue to
    compare against zero.  steady (the default at logit 64, see NO CANCELLATION above): dO keeps its sign per channel."""
    steady = amp < 8 if steady is None else steady
    rng = np.random.default_rng(seed)
    had, pos = hadamard16(), single_positions(Lk)
    q, k = np.zeros((B, H, Lq, 16)), np.zeros((B, H, Lk, 16))
    v = _ints(rng, (B, H, Lk, 16), -8, 8, nonzero=True)
    do, _ = _grad_out(rng, B, H, Lq, steady)
    o, dv = np.zeros_like(q), np.zeros_like(v)
    for b in range(B):
        for h in range(H):
            bh = b * H + h
            code = query_code(Lq, bh)
            sel = np.array([pos[(j + 5 * bh) % 16] for j in range(16)])  # key of code j
            k[b, h, sel] = amp * had
            q[b, h] = amp * had[code]
            o[b, h] = v[b, h, sel[code]]
            np.add.at(dv[b, h], sel[code], do[b, h])
    zq, zk = np.zeros_like(q), np.zeros_like(k)
    return _pack("single", H, q, k, v, do, dict(o=o, dq=zq, dk=zk, dv=dv))


def tie_case(B, H, Lq, Lk, seed=0, amp=4, steady=None):
    """Two selected keys per code.  d = V_a - V_b is in {-1, 0, 1} per channel, so x = dO.d has |x| <= 128 and dS = +-x / 16 is
    exact in bf16 whatever the last bits of the hardware's exp(64 - lse) are (it lands within 1e-5 of 1/2, bf16 rounds that
    away).  steady (the default at logit 64, see NO CANCELLATION above): d takes the sign of dO's channel, so x >= 0 and the sums
    over queries in dK and dV only grow; |x| is moved off the powers of two, because dQ = x/4 h - x/4 h passes through x/4."""
    steady = amp < 8 if steady is None else steady
    rng = np.random.default_rng(seed + 1)
    had, pairs = hadamard16(), tie_pairs(Lk)
    n = len(pairs)
    q, k = np.zeros((B, H, Lq, 16)), np.zeros((B, H, Lk, 16))
    v = _ints(rng, (B, H, Lk, 16), -7, 7)
    do, sign = _grad_out(rng, B, H, Lq, steady)
    o, dq, dk, dv = np.zeros_like(q), np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    for b in range(B):
        for h in range(H):
            bh = b * H + h
            code = query_code(Lq, bh, n)
            ab = np.array([pairs[(j + bh) % n] for j in range(n)])  # keys (a, b) of code j
            ka, kb = ab[:, 0], ab[:, 1]
            d = sign[b, h] * _ints(rng, (n, 16), 0, 1) if steady else _ints(rng, (n, 16), -1, 1)
            v[b, h, kb] = v[b, h, ka] - d
            k[b, h, ka] = k[b, h, kb] = amp * had[:n]
            q[b, h] = amp * had[code]
            va, vb = v[b, h, ka[code]], v[b, h, kb[code]]  # per query
            if steady:
                for qi in range(Lq):
                    chans = np.flatnonzero(d[code[qi]])
                    while _is_pow2((do[b, h, qi] * d[code[qi]]).sum()):  # one step up where there is room, else one down
                        room = [c for c in chans if abs(do[b, h, qi, c]) < 8]
                        c, step = (room[0], 1) if room else (chans[0], -1)
                        do[b, h, qi, c] += step * sign[b, h, c]
            o[b, h] = (va + vb) / 2
            ds = (do[b, h] * (va - vb)).sum(1) / 16        # at key a; minus that at key b
            np.add.at(dk[b, h], ka[code], ds[:, None] * q[b, h])
            np.add.at(dk[b, h], kb[code], -ds[:, None] * q[b, h])
            np.add.at(dv[b, h], ka[code], do[b, h] / 2)
            np.add.at(dv[b, h], kb[code], do[b, h] / 2)
    return _pack("tie", H, q, k, v, do, dict(o=o, dq=dq, dk=dk, dv=dv))


def weight_rounding_margin(Lk):
    """Distance of 1 / Lk from the nearest bf16 rounding boundary, relative to 1 / Lk (1 / 512 for a power of two)."""
    m, _ = np.frexp(1.0 / Lk)
    s = m * 256.0  # [128, 256): one unit = one bf16 ulp
    return abs(s - np.floor(s) - 0.5) / s


MARGIN = 1e-4  # the hardware's log and exp are good to ~1e-6 relative: a weight this far from a boundary rounds one way only


def uniform_weights(Lk):
    """The bf16 values exp(-lse) may round to when every weight is 1 / Lk: bf16(1 / Lk), and the bf16 number on the other side
    of the rounding boundary where 1 / Lk lies within MARGIN of it (Lk = 513: 1 / 513 = 255.501 / 256 x 2^-9)."""
    m, e = np.frexp(1.0 / Lk)
    s = m * 256.0
    lo = np.floor(s)
    near, far = (lo + 1, lo) if s - lo > 0.5 else (lo, lo + 1)
    ws = (float(np.ldexp(near, e - 8)),)
    assert ws[0] == float(bf16_round(1.0 / Lk))
    return ws + ((float(np.ldexp(far, e - 8)),) if weight_rounding_margin(Lk) < MARGIN else ())


def nomatch_case(B, H, Lq, Lk, seed=0):
    """Q = 0: uniform weights over the Lk valid keys.  O = bf16(w sum_keys V) and dV = bf16(w sum_queries dO) with
    w = bf16(1 / Lk); dK = dS^T Q = 0.  Products w x integer and their sums over at most 2 600 keys span fewer than 24 bits:
    exact in fp32 in any order.  (dQ = dS K depends on every rounding of dS; it is not part of this case.)
    `alt` holds the same closed forms for the second candidate of uniform_weights(Lk), where there is one."""
    rng = np.random.default_rng(seed + 2)
    base = single_case(B, H, Lq, Lk, seed)
    k = _heads(base["k"].double().numpy(), H)
    q = np.zeros((B, H, Lq, 16))
    v, do = _ints(rng, (B, H, Lk, 16), -8, 8), _ints(rng, (B, H, Lq, 16), -8, 8)
    packs = []
    for w in uniform_weights(Lk):
        o = np.broadcast_to(w * v.sum(2, keepdims=True), q.shape).copy()
        dv = np.broadcast_to(w * do.sum(2, keepdims=True), v.shape).copy()
        packs.append(_pack("nomatch", H, q, k, v, do, dict(o=o, dk=np.zeros_like(k), dv=dv)))
    packs[0]["alt"] = [p["expect"] for p in packs[1:]]
    return packs[0]


def gaussian_case(B, H, Lq, Lk, seed=0, std=0.5):
    g = torch.Generator().manual_seed(seed)
    E = H * 16
    q, k, v, do = [(torch.randn(B, L, E, generator=g) * std).to(torch.bfloat16) for L in (Lq, Lk, Lk, Lq)]
    return dict(name="gauss", H=H, q=q, k=k, v=v, do=do)


def reference(q, k, v, do, H, keep=None, p=0.0, scale=SCALE, rounded=True):
    """fp64 attention forward and backward on [B, L, H*16] tensors; keep: bool [B, H, Lq, Lk].  rounded: with the kernels'
    rounding points (weights, O and dS go through bf16; results rounded to bf16 once).  Returns o, dq, dk, dv as [B, L, H*16]
    fp64, lse [B, H, Lq] and the softmax weights p [B, H, Lq, Lk]."""
    rnd = bf16_round if rounded else (lambda x: x)
    B, Lq, E = q.shape

    def heads(t):
        return t.double().view(B, -1, H, 16).transpose(1, 2)

    def back(t):
        return t.transpose(1, 2).reshape(B, -1, E)

    hq, hk, hv, hdo = heads(q), heads(k), heads(v), heads(do)
    s = hq @ hk.transpose(-1, -2) * scale
    lse = torch.logsumexp(s, -1)
    pw = torch.exp(s - lse[..., None])
    drop = 1.0 if keep is None else torch.as_tensor(keep).double() / (1.0 - p)
    a = rnd(pw * drop)
    o = rnd(a @ hv)
    d = (hdo * o).sum(-1, keepdim=True)
    da = hdo @ hv.transpose(-1, -2) * drop
    ds = rnd(pw * (da - d) * scale)
    return dict(o=back(o), dq=back(rnd(ds @ hk)), dk=back(rnd(ds.transpose(-1, -2) @ hq)), dv=back(rnd(a.transpose(-1, -2) @ hdo)),
                lse=lse, p=pw)


def exact_mismatch(got, want, tiny=TINY):
    """Compare a result with a closed form: bit-equal (as values) to bf16(want) where that is non-zero, below `tiny` in
    magnitude where it is zero (tiny = 0: exactly zero).  Returns (number of wrong elements, largest |difference| among them)."""
    got = torch.as_tensor(got).detach().cpu().double()
    w = bf16_round(want)
    assert got.shape == w.shape, (got.shape, w.shape)
    bad = torch.where(w != 0, got != w, ~((got.abs() < tiny) | (got == 0)))
    return int(bad.sum()), float((got - w).abs()[bad].max()) if bool(bad.any()) else 0.0


# ------------------------------------------------------------------------------------------------ dropout hash
def eff_seed(seed, counter=0):
    """Host seed mixed with the device step counter, in 64-bit wrap-around arithmetic."""
    return (int(seed) + int(counter) * SEED_STEP) & M64


def thresh24(p):
    return np.uint32(np.float32(p) * np.float32(16777216.0))


def keep_hash(index, seed):
    """The 32-bit counter hash of csrc/attn.hip keep() on uint32 element indices; returns the 24-bit value compared with
    thresh24."""
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        x = index.astype(np.uint32) ^ lo
        x = x * np.uint32(0x9E3779B1)
        x ^= x >> np.uint32(15)
        x = x + hi
        x = x * np.uint32(0x85EBCA77)
        x ^= x >> np.uint32(13)
        x = x * np.uint32(0xC2B2AE3D)
        x ^= x >> np.uint32(16)
    return x >> np.uint32(8)


def keep_mask(B, H, Lq, Lk, p, seed, counter=0):
    """bool [B, H, Lq, Lk]: element ((b*H + h)*Lq + q)*Lk + key (mod 2^32) is kept."""
    index = (np.arange(B * H * Lq * Lk, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return (keep_hash(index, eff_seed(seed, counter)) >= thresh24(p)).reshape(B, H, Lq, Lk)
