# -*- coding: utf-8 -*-
"""The attention visibility census (test infrastructure): a one-layer model whose residual stream spells out, per row and per head,
WHICH keys the attention read — and the independent integer rule saying which keys it should have read.

The model (CensusModel.weights): token t has class c(t) in [0, C), C = n_kv_heads * head_dim; embed[t] is one-hot at hidden dim c(t);
q_proj = 0 (and a zero q/k/v bias on a qkv_bias shape), so every visible key gets the same softmax weight whatever k_proj (seeded
random) produces; v_proj carries class c into V lane c (kv head c // head_dim, lane c % head_dim); o_proj copies the n_heads * head_dim
attention lanes into hidden dims of their own; gate / up / down = 0 and every norm weight is 1.  After the layer, the lanes of head h
in row r hold s * w[c] / N: w = class histogram of the keys row r saw through h's kv head, N = all keys it saw, s = the one value the
input norm gives a one-hot row.  Normalised by their own sum the lanes give the histogram back: est = lanes * n / sum(lanes), n =
sum(w).  Every weight is 0, 1 or a bf16 / fp16-exact random number.

Two hidden layouts (la_llama_config admits hidden <= 8192):
  'disjoint'  hidden = C + n_heads * head_dim: class dims first, attention lanes after them (every shape that fits)
  'overlap'   hidden = n_heads * head_dim: the class dims ARE the first attention lanes; the row's own embedding sits on one lane
              of one head, which is subtracted for the normalisation and dropped from the comparison (40 / 40 heads at head_dim 128)

The bar (census_check): max |est - w| < 0.25.  A count passes through at most three 16-bit roundings (P, the attention output, the
residual store): relative 3 * 2^-9; with every class count <= 32 (asserted) a correct kernel deviates by at most ~0.19, while one
wrong (row, key) bit of class a moves that count by (n - w_a) / (n + 1) (gained key) or (n - w_a) / (n - 1) (lost key): at least 0.5
whenever class a holds fewer than half of the keys the head sees (2 w_a + 1 <= n).  The blind spot: a head is normalised by its own
lane sum, so when EVERY key it sees has class a (n = w_a) a gained or lost key of that class moves nothing; such a pair shows
through any row or head that sees a second class, which with the seeded classes is every row past the first few keys.

expected_visible is written from the documented semantics alone (a row sees the committed keys of its own slot — within `window`
positions of its own position nkeys + depth - 1 when there is a window — plus its ancestors and itself among the fresh rows); it
takes no engine output."""
import numpy as np
import torch

BAR = 0.25
COUNT_CAP = 32
GROUPS = 8          # class groups (class % GROUPS) of the slot-isolation tests


def popcount(x):
    return bin(int(x)).count('1')


def expected_visible(nkeys, rowmasks, window=0):
    """-> bool [R, nkeys + F].  rowmasks[r] = Python int, bit j set <=> fresh row j (of the same tree / chain, however many blocks it
    spans: F = the highest bit any row names, at least R) is an ancestor of row r or r itself.  Columns 0 .. nkeys - 1 are the committed keys
    of the row's slot by position, the rest the fresh rows.  window > 0: a committed key j is visible iff pos_row - j <= window,
    pos_row = nkeys + depth - 1, depth = popcount(rowmask)."""
    rowmasks = [int(m) for m in rowmasks]
    R = len(rowmasks)
    F = max([R] + [m.bit_length() for m in rowmasks])
    vis = np.zeros((R, nkeys + F), dtype=bool)
    for r, m in enumerate(rowmasks):
        lo = 0
        if window > 0:
            lo = max(0, nkeys + popcount(m) - 1 - window)          # pos_row - j <= window  <=>  j >= pos_row - window
        vis[r, lo:nkeys] = True
        j = 0
        while m:
            if m & 1:
                vis[r, nkeys + j] = True
            m >>= 1
            j += 1
    return vis


def wide_rowmasks(rm):
    """uint64 [T] or [T][W] (word w = tree columns 64 w ...) -> list of Python ints"""
    rm = np.asarray(rm, dtype=np.uint64)
    if rm.ndim == 1:
        rm = rm[:, None]
    return [sum(int(rm[r, w]) << (64 * w) for w in range(rm.shape[1])) for r in range(rm.shape[0])]


class CensusStats(object):
    """(row, head) checks made and the worst deviation seen, per test"""

    def __init__(self, name):
        self.name, self.checks, self.worst = name, 0, 0.0

    def __str__(self):
        return f'[census] {self.name}: {self.checks} (row, head) checks, worst deviation {self.worst:.4f} (bar {BAR})'


class CensusModel(object):
    def __init__(self, n_heads, n_kv_heads, head_dim=128, window=0, vocab=None, seed=0, lm_head='zero', qkv_bias=True, n_layers=1):
        assert n_heads % n_kv_heads == 0 and lm_head in ('zero', 'perm')
        self.nh, self.nkv, self.hd, self.window = n_heads, n_kv_heads, head_dim, int(window)
        self.C = n_kv_heads * head_dim
        self.lanes = n_heads * head_dim
        self.layout = 'disjoint' if self.C + self.lanes <= 8192 else 'overlap'
        self.hidden = self.C + self.lanes if self.layout == 'disjoint' else self.lanes
        self.lane0 = self.C if self.layout == 'disjoint' else 0
        self.vocab = int(vocab) if vocab else min(max(512, 2 * self.C), 2048)
        assert self.vocab % 32 == 0 and self.hidden % 32 == 0
        self.ffn = 512
        self.seed, self.head_kind, self.qkv_bias = seed, lm_head, bool(qkv_bias)
        rs = np.random.RandomState(1000 + seed)
        # token -> class: a seeded permutation of the classes, the second lap over the vocabulary shifted by 7
        perm = rs.permutation(self.C)
        t = np.arange(self.vocab)
        self.cls = perm[(t + 7 * (t // self.C)) % self.C].astype(np.int64)
        # the chain alphabet: tokens whose class is theirs alone among the alphabet.  succ (the permutation head) is one cycle per
        # class GROUP (class % GROUPS): a slot fed from one group's tokens keeps emitting that group's tokens, so that slots with
        # disjoint groups have disjoint classes and any count in a foreign class is a leak
        self.alphabet = min(self.C, self.vocab)
        self.succ_a = np.zeros(self.alphabet, dtype=np.int64)
        for g in range(GROUPS):
            members = np.nonzero(self.cls[:self.alphabet] % GROUPS == g)[0]
            order = members[rs.permutation(len(members))]
            self.succ_a[order] = np.roll(order, -1)
        self._tok_of_cls = np.full(self.C, -1, dtype=np.int64)
        self._tok_of_cls[self.cls[:self.alphabet]] = np.arange(self.alphabet)
        assert lm_head == 'zero' or self.layout == 'disjoint', 'the permutation head reads class dims no attention lane shares'

    def succ(self, tok):
        """the token the permutation head emits after `tok` (any token: it goes by the class)"""
        return int(self.succ_a[self._tok_of_cls[self.cls[int(tok)]]])

    def chain(self, tok, n):
        out = []
        for _ in range(n):
            tok = self.succ(tok)
            out.append(tok)
        return out

    def group_tokens(self, g):
        """the tokens of class group g (class % GROUPS == g)"""
        return np.nonzero(self.cls % GROUPS == g)[0]

    def chain_tree(self, rs, root, depth, T, tokens=None):
        """A DFS-ordered tree of T rows for the fused accept: row 0 = root, rows 1 .. depth its successor chain (each the child of the
        one before), the rest decoys hung under random rows of the current DFS path whose token is NOT their parent's successor
        (drawn from `tokens`, default the whole vocabulary).  -> (ids int32 [T], rowmask uint64 [T])"""
        assert 1 <= depth + 1 <= T <= 64
        tokens = np.arange(self.vocab) if tokens is None else np.asarray(tokens)
        ids = [int(root)] + self.chain(root, depth)
        masks = [(2 << i) - 1 for i in range(depth + 1)]
        stack = list(range(depth + 1))
        for i in range(depth + 1, T):
            while len(stack) > 1 and rs.rand() < 0.4:
                stack.pop()
            p = stack[-1]
            tok = int(tokens[rs.randint(len(tokens))])
            while tok == self.succ(ids[p]):
                tok = int(tokens[rs.randint(len(tokens))])
            ids.append(tok)
            masks.append(masks[p] | (1 << i))
            stack.append(i)
        return np.asarray(ids, dtype=np.int32), np.asarray(masks, dtype=np.uint64)

    def shape(self):
        from painlessinferenceacceleration_amd.llama_engine import LlamaShape
        return LlamaShape(1, self.hidden, self.nh, self.nkv, self.ffn, self.vocab, 1e-5, head_dim=self.hd,
                          sliding_window=self.window, qkv_bias=self.qkv_bias)

    def weights(self, dtype=torch.bfloat16):
        rs = np.random.RandomState(2000 + self.seed)
        C, hid, hd = self.C, self.hidden, self.hd
        sd = {}
        emb = torch.zeros(self.vocab, hid)
        emb[torch.arange(self.vocab), torch.from_numpy(self.cls)] = 1.0
        sd['model.embed_tokens.weight'] = emb
        p = 'model.layers.0.'
        sd[p + 'self_attn.q_proj.weight'] = torch.zeros(self.lanes, hid)
        # multiples of 1/64 in [-2, 2]: exact in bf16 and fp16
        sd[p + 'self_attn.k_proj.weight'] = torch.from_numpy(rs.randint(-128, 129, size=(C, hid)).astype(np.float32) / 64.0)
        v = torch.zeros(C, hid)
        v[torch.arange(C), torch.arange(C)] = 1.0
        sd[p + 'self_attn.v_proj.weight'] = v
        o = torch.zeros(hid, self.lanes)
        o[self.lane0 + torch.arange(self.lanes), torch.arange(self.lanes)] = 1.0
        sd[p + 'self_attn.o_proj.weight'] = o
        if self.qkv_bias:
            for nm, n in (('q', self.lanes), ('k', C), ('v', C)):
                sd[p + f'self_attn.{nm}_proj.bias'] = torch.zeros(n)
        sd[p + 'mlp.gate_proj.weight'] = torch.zeros(self.ffn, hid)
        sd[p + 'mlp.up_proj.weight'] = torch.zeros(self.ffn, hid)
        sd[p + 'mlp.down_proj.weight'] = torch.zeros(hid, self.ffn)
        sd[p + 'input_layernorm.weight'] = torch.ones(hid)
        sd[p + 'post_attention_layernorm.weight'] = torch.ones(hid)
        sd['model.norm.weight'] = torch.ones(hid)
        head = torch.zeros(self.vocab, hid)
        if self.head_kind == 'perm':
            a = np.arange(self.alphabet)
            head[torch.from_numpy(self.succ_a[a]), torch.from_numpy(self.cls[a])] = 1.0
        sd['lm_head.weight'] = head
        return {k: t.to(dtype) for k, t in sd.items()}

    # ------------------------------------------------------------------------------------------------ readout
    def histogram(self, vis, key_tokens):
        """vis bool [R, K], key_tokens int [K] -> int64 [R, C]: the class histogram of the keys each row sees"""
        vis = torch.as_tensor(np.asarray(vis), dtype=torch.float64)
        kc = torch.from_numpy(self.cls[np.asarray(key_tokens, dtype=np.int64)])
        assert vis.shape[1] == kc.shape[0], (vis.shape, kc.shape)
        w = torch.zeros(vis.shape[0], self.C, dtype=torch.float64)
        w.index_add_(1, kc, vis)
        assert float(w.max()) <= COUNT_CAP, f'class count {int(w.max())} > {COUNT_CAP}: the bar of the census holds for counts up to {COUNT_CAP}'
        return w

    def estimate(self, h, row_tokens, w):
        """h [R, hidden] (the residual stream after the layer), row_tokens [R], w [R, C] expected histogram
        -> (est [R, nh, hd], want [R, nh, hd], keep bool [R, nh, hd])"""
        R = h.shape[0]
        nh, hd, rep = self.nh, self.hd, self.nh // self.nkv
        lanes = h.detach().to('cpu', torch.float64)[:, self.lane0:self.lane0 + self.lanes].reshape(R, nh, hd).clone()
        want = w.reshape(R, self.nkv, 1, hd).expand(R, self.nkv, rep, hd).reshape(R, nh, hd).clone()
        keep = torch.ones(R, nh, hd, dtype=torch.bool)
        if self.layout == 'overlap':
            own = torch.from_numpy(self.cls[np.asarray(row_tokens, dtype=np.int64)])
            r = torch.arange(R)
            keep[r, own // hd, own % hd] = False             # embedding + lane on one dim: out of the sum and of the comparison
        n = (want * keep).sum(-1, keepdim=True)
        s = (lanes * keep).sum(-1, keepdim=True)
        est = torch.where(s > 0, lanes * n / s.clamp_min(1e-30), torch.zeros_like(lanes))
        # lanes that hold something where no key of the kv head's classes is visible: est would be 0 * x; report them as a full count
        ghost = (n == 0) & (lanes.abs() > 0)
        est = torch.where(ghost, torch.ones_like(est), est)
        return est, want, keep


def census_check(cm, h, row_tokens, vis, key_tokens, what, stats=None):
    """Compare the residual stream h [R, hidden] of R rows with the keys they should have seen (vis bool [R, K] over key_tokens [K]).
    Raises AssertionError naming (path, row, head, class -> key positions)."""
    key_tokens = np.asarray(key_tokens, dtype=np.int64)
    vis = np.asarray(vis, dtype=bool)
    w = cm.histogram(vis, key_tokens)
    est, want, keep = cm.estimate(h, row_tokens, w)
    dev = ((est - want).abs() * keep)
    n_rows = dev.shape[0]
    worst = float(dev.max()) if dev.numel() else 0.0
    if stats is not None:
        stats.checks += n_rows * cm.nh
        stats.worst = max(stats.worst, worst)
    if not worst < BAR:
        r, hh, ln = np.unravel_index(int(dev.reshape(-1).argmax()), tuple(dev.shape))
        c = (hh // (cm.nh // cm.nkv)) * cm.hd + ln
        of_class = np.nonzero(cm.cls[key_tokens] == c)[0]
        seen = [int(k) for k in of_class if vis[r, k]]
        hidden_ = [int(k) for k in of_class if not vis[r, k]]
        raise AssertionError(f'{what}: row {r} head {hh} class {c}: read {float(est[r, hh, ln]):.3f} keys, expected {int(want[r, hh, ln])} '
                             f'(deviation {worst:.3f} >= {BAR}); keys of that class the row should see: {seen}; keys of that class it '
                             f'should NOT see: {hidden_} (key index = position among {vis.shape[1]} keys, committed first)')
    return worst
