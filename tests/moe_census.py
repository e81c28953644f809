# -*- coding: utf-8 -*-
"""The MoE routing census (test infrastructure): a Mixtral-shaped model whose residual stream spells out, per row, WHICH experts ran on
that row's own activation and with WHAT weight — and the independent rule saying what it should spell.  Every checked number is exact
(single-term dot products, 16-bit-exact constants, zeros elsewhere): the comparison is equality, not a tolerance.

The model (MoeCensusModel.weights): token t has class c(t) in [0, C) (a seeded permutation, vocab = C); embed[t] is one-hot at hidden
dim c(t); v_proj = o_proj = 0, so attention adds nothing (q / k are seeded random); every norm weight is 1.  After the post-attention
norm (norm_cast_first, as tests.tiny_model.moe_shape) a row is s * onehot(c), s = round16(rsqrt(1 / hidden + eps)) the one value the
norm gives a one-hot row.  Classes fall into routing GROUPS of one logit pattern each: the router row Wr[e][c] = round16(target / s) of
the class's group, and the logit the row really gets, L[c][e] = round16(s * Wr[e][c]), is a 16-bit value by construction (equal targets
give equal logits: ties are exact).  Expert e: gate[f = c][k = c] = g_e, up[f = c][k = c] = u_e, down writes d_e into the expert's own
lane block (hidden dim C + e C + c) and q_e into a shared sum-lane block (C + E C + c); everything else is 0; hidden = (E + 2) C.
Every constant is a small multiple of a power of two, exact in bf16 and fp16.

After the last layer, row t (class c) must hold: 1 at dim c; in the lane block of a routed expert e, at lane c,
round16(round16(a_e d_e) w[t][e]), a_e = round16(round16(silu(round16(g_e s))) round16(u_e s)); at sum lane c the fold of
round16(round16(a_e q_e) w[t][e]) over the routed experts in expert-index order, rounded to 16 bits after every add (index_add_ into a
16-bit buffer); exactly 0 everywhere else.  A nonzero at another class lane means the row got another row's result (gather / perm /
pos); a nonzero in the block of an expert the row is not routed to, that the expert ran on it or a stale slab was read.  The routing
weights must equal softmax over the E logits -> top-k -> renormalise -> round16, ties to the LOWEST expert index (the rule
la_common.h::moe_router_tail documents; torch.topk's choice among equals is unspecified, so the oracle cannot judge tie rows).

MoeCensusModel.expected takes classes only — no engine output.  It is written in float64 with explicit 16-bit roundings; the generator
ASSERTS (on the CPU, at construction) the margins that make float64 and the kernels' fp32 agree after rounding: no routing weight and
no silu value lies within 2^-16 relative of a 16-bit rounding boundary (the fp32 chains err below ~2^-19), nor does s.

The blind spot: two live rows of one step that share a class share their group, hence their experts, and are indistinguishable — a
swap between them moves nothing.  The generator therefore hands every live row of a step a class of its own (MoeCensusModel.draw), so
no expert's row list holds two rows of one class; a step can check at most C live rows."""
import numpy as np
import torch

MARGIN = 2.0 ** -16
MAX_E = 8            # LA_MOE_MAX_E: the width of a route_weights row


def round16(x, dtype):
    """float64 (array / tensor / scalar) -> the nearest `dtype` value, as float64 (through fp32, which is where the kernels hold it)"""
    return torch.as_tensor(x, dtype=torch.float64).to(torch.float32).to(dtype).to(torch.float64)


def boundary_margin(v, dtype):
    """relative distance of |v| (float64 tensor, nonzero normal values) from the nearer of the two rounding boundaries around round16(v)"""
    a = torch.as_tensor(v, dtype=torch.float64).abs().reshape(-1)
    r = a.to(torch.float32).to(dtype)
    bits = r.view(torch.int16)
    up, dn = (bits + 1).view(dtype).to(torch.float64), (bits - 1).view(dtype).to(torch.float64)
    r = r.to(torch.float64)
    return torch.minimum((a - (r + up) / 2).abs(), (a - (r + dn) / 2).abs()) / a


def _tiny(dtype):
    """below this a positive value rounds to 0 in `dtype` with a factor 2^10 to spare (half the smallest subnormal / 1024)"""
    return (2.0 ** -134 if dtype == torch.bfloat16 else 2.0 ** -25) / 1024.0


def route_rule(logits, top_k, dtype):
    """logits float64 [G, E] (16-bit values) -> (w float64 [G, E]: round16 routing weights, 0 = not routed; sel bool [G, E]; raw float64
    [G, E]: the unrounded weights of the selected experts).  Ties go to the lowest expert index."""
    L = torch.as_tensor(logits, dtype=torch.float64)
    G, E = L.shape
    p = torch.softmax(L, dim=-1)
    sel = torch.zeros(G, E, dtype=torch.bool)
    for g in range(G):
        order = sorted(range(E), key=lambda e: (-float(L[g, e]), e))          # by logit, then the lowest index: softmax is monotone
        sel[g, order[:top_k]] = True
    raw = torch.where(sel, p, torch.zeros_like(p))
    raw = raw / raw.sum(-1, keepdim=True)
    w = torch.where(raw < _tiny(dtype), torch.zeros_like(raw), round16(raw, dtype))
    return w, sel, raw


def tie_rows(logits, top_k):
    """bool [G]: the k-th and (k + 1)-th largest logits are equal — the rows whose expert SET depends on the tie rule"""
    L = torch.as_tensor(logits, dtype=torch.float64)
    if top_k >= L.shape[1]:
        return torch.zeros(L.shape[0], dtype=torch.bool)
    s = torch.sort(L, dim=-1, descending=True).values
    return s[:, top_k - 1] == s[:, top_k]


class MoeCensusStats(object):
    """(row, expert) cells and routing weights checked, per test"""

    def __init__(self, name):
        self.name, self.cells, self.weights, self.rows, self.dead = name, 0, 0, 0, 0

    def __str__(self):
        return (f'[moe census] {self.name}: {self.rows} live rows, {self.cells} (row, expert) cells and {self.weights} routing weights '
                f'checked for equality, {self.dead} dead rows')


# SwiGLU / down constants per expert: multiples of 1/256 (gate, up: the operand is s ~ sqrt(hidden)) and of 1/64 (down): <= 8
# significant bits, exact in bf16 and fp16
_G256 = (9, -7, 13, 5, -11, 15, 7, -13, 11, -5, 17, 3, -9, 19, -15, 21)
_U256 = (7, 11, -5, 9, 13, -9, 5, -7)
_D64 = (64, -96, 80, 48, -112, 72, 104, -56)
_Q64 = (67, -113, 29, 101, -59, 127, -37, 89)


class MoeCensusModel(object):
    """E experts, top_k, storage dtype, C classes.  plant: rows a step can draw from each WINDOW group j (experts j .. j + top_k - 1 mod E;
    one group when top_k = E) — the pool of group j holds max(plant[j], 4) classes; the remaining classes are dealt to the edge groups
    (an exact tie at the top-k boundary, a tie among all experts, a logit gap of ~100) and to seeded random patterns.  layers = 2: layer 0
    runs experts whose down projection is 0 behind a router of its own (another seed), the census is read after layer 1."""

    def __init__(self, E, top_k, dtype, C=128, plant=None, seed=0, layers=1, n_random=4):
        assert 1 <= top_k <= E <= MAX_E and C % 128 == 0 and layers in (1, 2)
        self.E, self.k, self.dtype, self.C, self.L = E, top_k, dtype, C, layers
        self.hidden, self.ffn, self.vocab = (E + 2) * C, max(512, C), C
        self.eps = 1e-5
        s64 = 1.0 / np.sqrt(1.0 / self.hidden + self.eps)
        assert float(boundary_margin(torch.tensor([s64]), dtype)) > MARGIN, 'the norm value of a one-hot row sits on a rounding boundary'
        self.s = float(round16(s64, dtype))
        rs = np.random.RandomState(7000 + 131 * seed + 17 * E + top_k)
        # ---- groups: (name, target logits); window groups first
        n_win = E if top_k < E else 1
        plant = list(plant) if plant is not None else [8] * n_win
        assert len(plant) == n_win, (len(plant), n_win)
        groups, pools = [], []
        for j in range(n_win):
            S = [(j + i) % E for i in range(top_k)]
            groups.append((f'window{j}', self._pattern(rs, S, E)))
            pools.append(max(int(plant[j]), 4))
        # the edge groups: a function of the random state each, redrawn (same structure, other values) until the weights clear the margin
        edges = []
        if top_k < E:
            order = [int(e) for e in rs.permutation(E)]
            ahead, a, b = order[:top_k - 1], min(order[top_k - 1:top_k + 1]), max(order[top_k - 1:top_k + 1])
            rest = [e for e in range(E) if e not in ahead and e not in (a, b)]

            def boundary_tie(r, third=None):
                """top_k - 1 experts clearly ahead, then equal logits on experts a < b (and `third`): exactly one of them is taken"""
                t = -(r.permutation(33)[:E] / 16.0 + 1.0)
                t[ahead] = r.permutation(17)[:top_k - 1] / 16.0 + 1.0
                t[[a, b] + ([third] if third is not None else [])] = r.randint(-8, 9) / 16.0
                return t
            edges.append(('tie at the boundary', boundary_tie))
            if rest:
                edges.append(('triple tie at the boundary', lambda r: boundary_tie(r, rest[-1])))
        if E >= 2:
            edges.append(('tie among all experts', lambda r: np.full(E, r.randint(-16, 17) / 16.0)))
            hi = int(rs.randint(E))

            def gap100(r):
                """the second weight underflows: one expert ~100 above the others, which differ among themselves (no tie anywhere)"""
                t = -50.0 - 0.5 * np.arange(E)
                t[hi] = 50.0
                return t
            edges.append(('gap 100', gap100))
        self.window_groups = list(range(n_win))
        self.edge_groups = {}
        left = C - sum(pools)
        assert left >= 0, f'plant needs {sum(pools)} classes, C = {C}'
        n_other = len(edges) + n_random
        per = left // n_other if n_other else 0
        assert per >= 2 or left == 0, f'{left} classes for {n_other} edge / random groups'
        for name, t in edges:
            self.edge_groups[name] = len(groups)
            groups.append((name, t))
            pools.append(per)
        self.random_groups = []
        for r in range(n_random):
            self.random_groups.append(len(groups))
            groups.append((f'random{r}', None))
            pools.append(per)
        pools[-1] += C - sum(pools)
        self.names = [g[0] for g in groups]
        self.pools = pools
        # ---- expert constants and what they make of s
        ge = [g / 256.0 for g in _G256]
        self.g, self.u = [], [u / 256.0 for u in _U256[:E]]
        for e in range(E):                              # the first gate constant whose silu clears the margin, per expert
            for cand in ge[e:] + ge[:e]:
                pre = round16(cand * self.s, dtype)
                if cand not in self.g and float(boundary_margin(torch.nn.functional.silu(pre), dtype)) > MARGIN:
                    self.g.append(cand)
                    break
            else:
                raise AssertionError('no gate constant clears the silu margin')
        self.d, self.q = [d / 64.0 for d in _D64[:E]], [q / 64.0 for q in _Q64[:E]]
        pre_g = round16(torch.tensor(self.g, dtype=torch.float64) * self.s, dtype)
        pre_u = round16(torch.tensor(self.u, dtype=torch.float64) * self.s, dtype)
        self.a = round16(round16(torch.nn.functional.silu(pre_g), dtype) * pre_u, dtype)         # [E]
        self.y_own = round16(self.a * torch.tensor(self.d, dtype=torch.float64), dtype)           # what down writes into the own lane
        self.y_sum = round16(self.a * torch.tensor(self.q, dtype=torch.float64), dtype)           # ... and into the sum lane
        assert bool((self.y_own != 0).all()) and bool((self.y_sum != 0).all())
        # ---- router tables, per layer: Wr = round16(target / s), the logits a row really gets L = round16(s * Wr); every group is
        # redrawn (an edge group: same structure, other values) until its weights clear the rounding margin; layer 0 of a two-layer model
        # gets seeded random patterns throughout
        self.Wr, self.logits, self.w, self.sel = [], [], [], []
        for layer in range(layers):
            lrs = np.random.RandomState(9000 + 977 * layer + seed) if layer < layers - 1 else rs
            Wr = torch.zeros(len(groups), E, dtype=torch.float64)
            last = layer == layers - 1
            for gi, (name, t) in enumerate(groups):
                designed = last and t is not None and not name.startswith('window')
                for attempt in range(200):
                    if designed:
                        tt = t(lrs)
                    elif last and name.startswith('window'):
                        tt = t if attempt == 0 else self._pattern(lrs, [(gi + i) % E for i in range(top_k)], E)
                    else:
                        tt = np.round(lrs.uniform(-2.5, 2.5, size=E) * 16) / 16
                    wr = round16(torch.from_numpy(np.asarray(tt, dtype=np.float64)) / self.s, dtype)
                    L1 = round16(self.s * wr, dtype)[None]
                    # designed groups keep their structure; the others must also make the sum lane depend on the expert order (top_k >= 3)
                    if self._clear(L1) and (designed or not last or top_k < 3 or self._fold_differs(L1)):
                        break
                else:
                    raise AssertionError(f'no pattern of group {name} clears the rounding margin')
                Wr[gi] = wr
            L = round16(self.s * Wr, dtype)
            w, sel, _ = route_rule(L, top_k, dtype)
            self.Wr.append(Wr); self.logits.append(L); self.w.append(w); self.sel.append(sel)
        self.ties = tie_rows(self.logits[-1], top_k)
        for name in ('tie at the boundary', 'triple tie at the boundary'):
            if name in self.edge_groups:
                assert bool(self.ties[self.edge_groups[name]]), name
        if 'gap 100' in self.edge_groups:
            wg = self.w[-1][self.edge_groups['gap 100']]
            assert float(wg.max()) == 1.0 and int((wg != 0).sum()) == 1, wg
        for j in self.window_groups:                     # the window groups route where they say
            want = sorted((j + i) % E for i in range(top_k))
            assert sorted(torch.nonzero(self.sel[-1][j]).flatten().tolist()) == want
        # ---- classes: group g owns a contiguous pool; token <-> class by a seeded permutation
        self.group_of = np.repeat(np.arange(len(groups)), pools)
        assert len(self.group_of) == C
        self.cls = np.random.RandomState(8000 + seed).permutation(C).astype(np.int64)          # token -> class
        self.tok_of = np.argsort(self.cls)                                                        # class -> token
        # every contribution of a routed expert with a nonzero weight is itself nonzero and normal: a routed cell never reads 0
        wmin = self.w[-1][self.w[-1] > 0].min()
        assert float(wmin * self.y_own.abs().min()) > 2.0 ** -13 and float(wmin * self.y_sum.abs().min()) > 2.0 ** -13

    @staticmethod
    def _pattern(rs, S, E):
        """target logits with the experts S ahead: distinct multiples of 1/16 in [0.5, 2.5] on S, in [-2.5, -0.5] elsewhere"""
        t = -(rs.permutation(33)[:E] / 16.0 + 0.5)
        t[S] = rs.permutation(33)[:len(S)] / 16.0 + 0.5
        return t

    def _fold_differs(self, L):
        """the sum-lane fold of a row with logits L [1, E] differs between ascending and descending expert order"""
        w = route_rule(L, self.k, self.dtype)[0][0]
        out = []
        for order in (range(self.E), reversed(range(self.E))):
            acc = None
            for e in order:
                if w[e] != 0:
                    c = round16(self.y_sum[e] * w[e], self.dtype).to(torch.float32)
                    acc = c if acc is None else (acc + c).to(self.dtype).to(torch.float32)
            out.append(float(acc))
        return out[0] != out[1]

    def _clear(self, L):
        _, sel, raw = route_rule(L, self.k, self.dtype)
        v = raw[sel]
        v = v[v >= _tiny(self.dtype)]
        assert bool((raw[sel] < _tiny(self.dtype)).logical_or(raw[sel] > 2.0 ** -12).all()), 'a routing weight between 0 and 2^-12'
        return bool((boundary_margin(v, self.dtype) > MARGIN).all())

    # ------------------------------------------------------------------------------------------------ model
    def shape(self):
        from painlessinferenceacceleration_amd.llama_engine import LlamaShape
        return LlamaShape(self.L, self.hidden, 2, 1, self.ffn, self.vocab, self.eps, rope_theta=1e6, head_dim=128, n_experts=self.E,
                          top_k=self.k, norm_cast_first=True)

    def weights(self):
        C, E, hid, dt = self.C, self.E, self.hidden, self.dtype
        rs = np.random.RandomState(2000)
        sd = {}
        emb = torch.zeros(self.vocab, hid)
        emb[torch.arange(self.vocab), torch.from_numpy(self.cls)] = 1.0
        sd['model.embed_tokens.weight'] = emb
        ar = torch.arange(C)
        for layer in range(self.L):
            p = f'model.layers.{layer}.'
            # multiples of 1/1024 in [-1/8, 1/8]: exact in bf16 and fp16, and small enough that q . k of rows s * onehot stays far inside fp16
            sd[p + 'self_attn.q_proj.weight'] = torch.from_numpy(rs.randint(-128, 129, size=(256, hid)).astype(np.float32) / 1024.0)
            sd[p + 'self_attn.k_proj.weight'] = torch.from_numpy(rs.randint(-128, 129, size=(128, hid)).astype(np.float32) / 1024.0)
            sd[p + 'self_attn.v_proj.weight'] = torch.zeros(128, hid)
            sd[p + 'self_attn.o_proj.weight'] = torch.zeros(hid, 256)
            sd[p + 'input_layernorm.weight'] = torch.ones(hid)
            sd[p + 'post_attention_layernorm.weight'] = torch.ones(hid)
            router = torch.zeros(E, hid)
            router[:, :C] = self.Wr[layer][torch.from_numpy(self.group_of)].t().to(torch.float32)       # Wr[e][c] of the class's group
            sd[p + 'block_sparse_moe.gate.weight'] = router
            for e in range(E):
                q = p + f'block_sparse_moe.experts.{e}.'
                w1, w3, w2 = torch.zeros(self.ffn, hid), torch.zeros(self.ffn, hid), torch.zeros(hid, self.ffn)
                w1[ar, ar] = self.g[e]
                w3[ar, ar] = self.u[e]
                if layer == self.L - 1:
                    w2[C + e * C + ar, ar] = self.d[e]
                    w2[C + E * C + ar, ar] = self.q[e]
                sd[q + 'w1.weight'], sd[q + 'w3.weight'], sd[q + 'w2.weight'] = w1, w3, w2
        sd['model.norm.weight'] = torch.ones(hid)
        sd['lm_head.weight'] = torch.zeros(self.vocab, hid)
        out = {k: t.to(dt) for k, t in sd.items()}
        for k, t in sd.items():
            assert torch.equal(out[k].to(torch.float32), t), f'{k} is not exact in {dt}'
        return out

    # ------------------------------------------------------------------------------------------------ rows of a step
    def draw(self, rs, counts, spare=0):
        """counts: {group index or edge-group name: rows} (+ `spare` rows from the random groups, round robin) -> tokens int32, in a
        seeded random order; every row a class of its own"""
        classes = []
        first = np.concatenate([[0], np.cumsum(self.pools)])
        want = {(self.edge_groups[g] if isinstance(g, str) else int(g)): int(n) for g, n in counts.items()}
        for i in range(spare):
            g = self.random_groups[i % len(self.random_groups)]
            want[g] = want.get(g, 0) + 1
        for g, n in want.items():
            assert n <= self.pools[g], f'group {self.names[g]} holds {self.pools[g]} classes, {n} rows asked'
            classes += list(first[g] + rs.permutation(self.pools[g])[:n])
        classes = np.asarray(classes, dtype=np.int64)[rs.permutation(len(classes))]
        assert len(set(classes.tolist())) == len(classes)
        return self.tok_of[classes].astype(np.int32)

    def draw_mixed(self, rs, n):
        """n tokens of n different classes over all groups; from 16 rows on, one class of every edge group is among them"""
        assert n <= self.C
        first = np.concatenate([[0], np.cumsum(self.pools)])
        lead = [int(first[g] + rs.randint(self.pools[g])) for g in self.edge_groups.values()] if n >= 16 else []
        rest = [int(c) for c in rs.permutation(self.C) if int(c) not in lead]
        classes = np.asarray((lead + rest)[:n], dtype=np.int64)[rs.permutation(n)]
        return self.tok_of[classes].astype(np.int32)

    def expert_counts(self, tokens, layer=-1):
        """rows per expert among `tokens`, counted from the expected routing (selected AND weight != 0: what a kernel can see)"""
        g = self.group_of[self.cls[np.asarray(tokens, dtype=np.int64)]]
        return (self.w[layer][torch.from_numpy(g)] != 0).sum(0).tolist()

    def is_tie(self, tokens):
        return self.ties[torch.from_numpy(self.group_of[self.cls[np.asarray(tokens, dtype=np.int64)]])]

    # ------------------------------------------------------------------------------------------------ the rule
    def expected(self, tokens, reverse=False):
        """tokens [R] -> (w [layers, R, E], h [R, hidden]) float64: the routing weights of every layer and the residual stream after the
        last layer.  reverse: the sum lane folded in DESCENDING expert order (the order-sensitivity condition only)."""
        tokens = np.asarray(tokens, dtype=np.int64)
        R, C, E, dt = len(tokens), self.C, self.E, self.dtype
        c = torch.from_numpy(self.cls[tokens])
        g = torch.from_numpy(self.group_of[self.cls[tokens]])
        w = torch.stack([wl[g] for wl in self.w])                                 # [layers, R, E]
        h = torch.zeros(R, self.hidden, dtype=torch.float64)
        r = torch.arange(R)
        h[r, c] = 1.0
        wl = w[-1]
        fold = torch.zeros(R, dtype=torch.float32)
        started = torch.zeros(R, dtype=torch.bool)
        for e in (reversed(range(E)) if reverse else range(E)):
            on = wl[:, e] != 0
            h[r, C + e * C + c] = torch.where(on, round16(self.y_own[e] * wl[:, e], dt), torch.zeros(R, dtype=torch.float64))
            contrib = round16(self.y_sum[e] * wl[:, e], dt).to(torch.float32)
            nxt = torch.where(started, (fold + contrib).to(dt).to(torch.float32), contrib)       # fp32 add, one rounding: as the buffer
            fold = torch.where(on, nxt, fold)
            started |= on
        h[r, C + E * C + c] = fold.to(torch.float64)
        return w, h

    def order_sensitive(self, tokens):
        """fraction of rows whose sum-lane fold differs when taken in reverse expert order"""
        a, b = self.expected(tokens)[1], self.expected(tokens, reverse=True)[1]
        return float((a != b).any(-1).float().mean())


def census_check(cm, h, rw, tokens, what, stats=None, n_dead=0, layers=None):
    """h [R + n_dead, hidden]: the residual stream of the R live rows `tokens` followed by n_dead dead rows of their block; rw [layers, R +
    n_dead, >= E]: the routing weights.  Equality with the rule on every element; raises AssertionError naming (path, row, what cell)."""
    tokens = np.asarray(tokens, dtype=np.int64)
    R, C, E = len(tokens), cm.C, cm.E
    w, want = cm.expected(tokens)
    if cm.k >= 3 and R >= 16:
        assert cm.order_sensitive(tokens) >= 0.25, f'{what}: the sum lanes of this step would not notice another expert order'
    h = h.detach().to('cpu', torch.float64)
    rw = rw.detach().to('cpu', torch.float64)
    assert h.shape[0] == R + n_dead and rw.shape[1] == R + n_dead, (what, h.shape, rw.shape, R, n_dead)
    for layer in (range(cm.L) if layers is None else layers):
        got = rw[layer, :R, :E]
        if not torch.equal(got, w[layer]):
            bad = torch.nonzero((got != w[layer]).any(-1)).flatten()
            t = int(bad[0])
            raise AssertionError(f'{what}: layer {layer} routing weights of row {t} (class {int(cm.cls[tokens[t]])}, group '
                                 f'{cm.names[cm.group_of[cm.cls[tokens[t]]]]}): got {got[t].tolist()}, expected {w[layer, t].tolist()} '
                                 f'(logits {cm.logits[layer][cm.group_of[cm.cls[tokens[t]]]].tolist()}); {len(bad)} rows differ')
        assert not bool(rw[layer, :R, E:].any()), f'{what}: layer {layer} weights past expert {E}'
        assert not bool(rw[layer, R:].any()), f'{what}: layer {layer}: a dead row carries a routing weight'
    live = h[:R]
    if not torch.equal(live, want):
        t, dim = (int(x) for x in torch.nonzero(live != want)[0])
        c = int(cm.cls[tokens[t]])
        blk, lane = (dim - C) // C, dim % C
        where = 'class dims' if dim < C else (f'sum lanes' if blk == E else f'lane block of expert {blk}')
        others = [int(i) for i in np.nonzero(cm.cls[tokens] == lane)[0]]
        raise AssertionError(f'{what}: row {t} (class {c}, group {cm.names[cm.group_of[c]]}, weights {w[-1, t].tolist()}): {where}, lane {lane}: got '
                             f'{float(live[t, dim])!r}, expected {float(want[t, dim])!r}; rows of class {lane} in this step: {others}; '
                             f'{int((live != want).sum())} elements differ in {int((live != want).any(-1).sum())} rows')
    if n_dead:
        assert not bool(h[R:, C:].any()), f'{what}: a dead row holds an expert output: rows {torch.nonzero(h[R:, C:].any(-1)).flatten().tolist()}'
    if stats is not None:
        stats.rows += R
        stats.dead += n_dead
        stats.cells += R * (E + 1)
        stats.weights += R * E * len(range(cm.L) if layers is None else layers)
