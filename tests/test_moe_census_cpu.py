# -*- coding: utf-8 -*-
"""The rule of tests/moe_census.py against the oracle (oracle.llama_oracle.OracleLlama, pinned to the reference) on the census model,
bf16 and fp16, on the CPU: on every tie-free row the residual stream after the last layer and the routing derived from the oracle's
router logits are EQUAL to what the rule expects.  If a rounding point differed, the oracle would win: the rule is the thing to
correct.  Rows whose k-th and (k + 1)-th logits tie are set aside (torch.topk's choice among equals is unspecified) and counted."""
import numpy as np
import pytest
import torch

from oracle import llama_oracle as lo
from tests.moe_census import MARGIN, MoeCensusModel, boundary_margin, round16, route_rule, tie_rows

DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(8, 2), (8, 1), (8, 4), (4, 3), (2, 2), (1, 1), (8, 5), (8, 8)]


def _oracle_routing(logits, top_k, dtype):
    """MixtralSparseMoeBlock's routing from the oracle's router logits -> [T, E] weights (0 = not routed), float64"""
    p = torch.softmax(logits, dim=1, dtype=torch.float)
    v, sel = torch.topk(p, top_k, dim=-1)
    v = (v / v.sum(dim=-1, keepdim=True)).to(dtype)
    out = torch.zeros(logits.shape, dtype=torch.float64)
    out.scatter_(1, sel, v.to(torch.float64))
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('E,top_k', SHAPES)
def test_rule_equals_the_oracle_on_every_tie_free_row(E, top_k, dtype):
    layers = 2 if (E, top_k) == (8, 2) else 1
    cm = MoeCensusModel(E, top_k, dtype, C=128, layers=layers)
    sd = cm.weights()
    oracle = lo.OracleLlama(cm.shape(), sd)
    oracle.trace_hidden = True
    rs = np.random.RandomState(5)
    tokens = cm.tok_of[rs.permutation(cm.C)]                       # every class once: every group, every edge
    T = len(tokens)
    oracle.forward(torch.from_numpy(tokens), torch.tril(torch.ones((T, T), dtype=torch.long)), None)
    w, h = cm.expected(tokens)
    ties = cm.is_tie(tokens)
    free = ~ties
    got_h = oracle.hidden_trace[-1].to(torch.float64)
    assert torch.equal(got_h[free], h[free]), torch.nonzero(got_h[free] != h[free])[:5]
    n_w = 0
    for layer in range(layers):
        logits = oracle.router_trace[layer]
        want_logits = cm.logits[layer][torch.from_numpy(cm.group_of[cm.cls[tokens]])]
        assert torch.equal(logits.to(torch.float64), want_logits), f'layer {layer}: the router logits are not the designed table'
        t_l = tie_rows(want_logits, top_k)
        got_w = _oracle_routing(logits, top_k, dtype)
        assert torch.equal(got_w[~t_l], w[layer][~t_l]), torch.nonzero(got_w[~t_l] != w[layer][~t_l])[:5]
        n_w += int((~t_l).sum()) * E
        # on a tie row the rule and the oracle may pick different experts, but the weights they hand out are the same multiset
        assert torch.equal(torch.sort(got_w[t_l], -1).values, torch.sort(w[layer][t_l], -1).values)
    print(f'[moe census] cpu rule vs oracle E {E} top_k {top_k} {dtype}: {int(free.sum())} rows compared with the oracle '
          f'({int(free.sum()) * (E + 1)} cells, {n_w} routing weights), {int(ties.sum())} tie rows set aside')
    assert int(free.sum()) >= T // 2
    if top_k < E:
        assert int(ties.sum()) > 0
    if top_k >= 3:
        assert cm.order_sensitive(tokens) >= 0.25


def test_the_tie_rule_is_the_lowest_index():
    """the documented rule (la_common.h::moe_router_tail: the earliest expert wins a tie), stated on its own"""
    w, sel, _ = route_rule(torch.tensor([[0.25, 0.25, 0.25, 0.25], [0.5, 1.0, 0.5, 0.5]], dtype=torch.float64), 2, torch.bfloat16)
    assert sel.tolist() == [[True, True, False, False], [True, True, False, False]]
    assert w[0].tolist() == [0.5, 0.5, 0.0, 0.0]


@pytest.mark.parametrize('dtype', DTYPES)
def test_generator_conditions(dtype):
    """the margins the equality rests on, and the planted counts, are asserted by the generator itself; here: that they are not vacuous"""
    plant = [0, 1, 62, 2, 63, 65, 64, 0]
    cm = MoeCensusModel(8, 2, dtype, C=384, plant=plant)
    rs = np.random.RandomState(1)
    tokens = cm.draw(rs, {j: n for j, n in enumerate(plant) if n})
    assert cm.expert_counts(tokens) == [0, 1, 63, 64, 65, 128, 129, 64]
    assert len(set(cm.cls[tokens].tolist())) == len(tokens)                     # the blind spot is kept out: a class of its own per row
    for layer in range(cm.L):
        _, sel, raw = route_rule(cm.logits[layer], cm.k, dtype)
        v = raw[sel]
        assert bool((boundary_margin(v[v > 2.0 ** -100], dtype) > MARGIN).all())
    pre = round16(torch.tensor(cm.g, dtype=torch.float64) * cm.s, dtype)
    assert bool((boundary_margin(torch.nn.functional.silu(pre), dtype) > MARGIN).all())
    g = cm.w[-1][cm.edge_groups['gap 100']]
    assert sorted(g.tolist())[-2:] == [0.0, 1.0]
    with pytest.raises(AssertionError):
        cm.draw(rs, {0: 5})                                                    # more rows than the group has classes
