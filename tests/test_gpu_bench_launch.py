# -*- coding: utf-8 -*-
"""GPU: `python bench.py --gpus N` called the way the driver calls the N = 1 command (no rank environment) spawns its own N
ranks and prints ONE JSON line.  On the 1-GPU box the ranks share the device (BENCH_SHARE_GPU=1) and the accepted-token
gather runs over gloo on host tensors (BENCH_DIST_BACKEND=gloo): the control flow of the N-rank job, not its transport."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize('strict', [False, True])
def test_bench_self_launches_two_ranks(strict):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR'):
        env.pop(k, None)
    env.update({'BENCH_SHARE_GPU': '1', 'BENCH_DIST_BACKEND': 'gloo'})
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '6', '--warmup', '2', '--layers', '2',
           '--no-cpu-baseline', '--secondary', '', '--full'] + (['--strict-gather'] if strict else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1000:], r.stderr[-3000:])
    j = json.loads(lines[0])
    assert j['n_gpus'] == 2 and j['scaling'] == 'weak' and j['steps'] == 6
    c = j['config']
    assert c['gather_mode'] == ('strict' if strict else 'split-phase')
    assert c['gather_transport'] == 'torch.distributed(gloo)' and c['rccl_ranks'] == 0      # the transport is named, never implied
    assert c['sequences'] == 2 and c['lookahead_equals_greedy'] is True
    assert c['gather_us_per_step'] >= 0 and c['slowest_rank_wait_us'] >= 0 and 'notes' in j
    assert any(ln.startswith('BENCH_DETAIL {') for ln in r.stdout.splitlines())      # the full record precedes the compact line


@pytest.mark.gpu
def test_bench_gathers_over_rccl_with_one_rank_per_gpu():
    """Multi-GPU readiness on the REAL transport: torch.distributed 'nccl' (= RCCL) for the control collectives and la_gather_accepted
    (ncclAllGather on the package's own communicator, csrc/la_comm.cpp) for the per-step gather, one rank per device — two ranks on two
    GPUs where the box has them.  RCCL refuses two ranks of one communicator on one device ("Duplicate GPU detected"), so a one-GPU box
    runs the same job as ONE rank (BENCH_FORCE_DIST=1): process group, communicator and the gather of every step, nothing emulated."""
    import torch
    import bench
    n = min(torch.cuda.device_count(), 2)
    env = bench.clean_rank_env()
    for k in ('BENCH_SHARE_GPU', 'BENCH_DIST_BACKEND', 'BENCH_FORCE_DIST'):
        env.pop(k, None)
    if n == 1:
        env['BENCH_FORCE_DIST'] = '1'
    args = ['--gpus', str(n), '--steps', '6', '--warmup', '2', '--layers', '2', '--no-cpu-baseline', '--secondary', '']
    r = subprocess.run(bench.self_launch_cmd(args, n, bench._free_port()), env=env, capture_output=True, text=True, timeout=420, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1000:], r.stderr[-3000:])
    j = json.loads(lines[0])
    c = j['config']
    assert j['n_gpus'] == n and j['steps'] == 6 and c['sequences'] == n and c['lookahead_equals_greedy'] is True
    assert c['gather_transport'] == 'la_gather_accepted(rccl)' and c['rccl_ranks'] == n and c['gather_mode'] == 'split-phase'
    assert c['gather_us_per_step'] is not None and c['slowest_rank_wait_us'] is not None


@pytest.mark.gpu
def test_bench_self_launches_two_ranks_and_runs_config4_as_its_own_multi_rank_job():
    """`python bench.py --gpus N --full` with no rank environment: N ranks of the headline workload, then
    BASELINE config 4 — Llama-2-13B, 4 sequences per GPU, batch-sharded over the N ranks — as its own N-rank job embedded under
    `secondary` (at --gpus 8 that leg is the default, tests/test_bench_helpers_cpu.py).  The box has one GPU, which at most a handful
    of processes may hold open at once: N = 2 ranks share it (the first job's ranks, the second job's ranks and this process overlap
    while the nested job starts) and the gather runs over gloo (control flow, not transport); both models are cut to 2 layers
    (--layers / --secondary-layers: launch-path test, not a metric)."""
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR'):
        env.pop(k, None)
    env.update({'BENCH_SHARE_GPU': '1', 'BENCH_DIST_BACKEND': 'gloo'})
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '1', '--layers', '2',
           '--secondary-layers', '2', '--secondary-multi', '13b:4', '--no-cpu-baseline', '--strict-gather', '--full']
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1000:], r.stderr[-3000:])
    j = json.loads(lines[0])
    assert j['n_gpus'] == 2 and j['scaling'] == 'weak' and j['config']['sequences'] == 2 and j['steps'] == 4
    assert j['config']['gather_mode'] == 'strict' and j['config']['rccl_ranks'] == 0
    sec = j['secondary']
    assert len(sec) == 1 and 'error' not in sec[0], sec
    leg = sec[0]
    assert leg['n_gpus'] == 2 and leg['sequences'] == 8 and leg['model'] == 'Llama-2-13B' and leg['n_layers'] == 2      # compact leg (bench.compact_leg)
    assert leg['equals_greedy'] is True and leg['gather_transport'] == 'torch.distributed(gloo)'
    assert leg['gather_us_per_step'] is not None and leg['slowest_rank_wait_us'] is not None
    assert len(lines[0]) < 8000                                  # the whole record fits the driver's captured 8 KB tail


def _bench_dump(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--layers', '2',
           '--no-cpu-baseline', '--secondary', '', '--dump-outputs', str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1000:], r.stderr[-3000:])
    j = json.loads(lines[0])
    assert j['steps'] == 3 and j['warmup'] == 1 and j['config']['lookahead_equals_greedy'] is True
    names = ('generated_tokens', 'last_step_tokens', 'last_step_logits', 'last_step_logit_rows')
    assert sorted(os.listdir(out_dir)) == sorted(n + '.npy' for n in names)
    assert sum(os.path.getsize(os.path.join(out_dir, n + '.npy')) for n in names) <= 64 << 20
    return {n: np.load(os.path.join(out_dir, n + '.npy')) for n in names}


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [1, 2])
def test_bench_dump_outputs_hold_the_last_timed_step_and_repeat_run_to_run(tmp_path, batch):
    """--dump-outputs DIR: after the timed steps bench.py writes what they computed — the emitted tokens, the last step's accepted
    tokens, and that step's logits per (sequence, tree row).  Seeded inputs: a second run of the same command writes the same arrays.
    The first accepted token of every sequence is the argmax of its tree root's logits (decisive synthetic weights: no near-ties)."""
    a = _bench_dump(tmp_path / 'a', '--batch', str(batch))
    b = _bench_dump(tmp_path / 'b', '--batch', str(batch))
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
    gen, last, lg, rows = a['generated_tokens'], a['last_step_tokens'], a['last_step_logits'], a['last_step_logit_rows']
    assert gen.shape[0] == last.shape[0] == batch and lg.shape == (rows.shape[0], 32000) and rows.shape[1] == 2
    for i in range(batch):
        n_gen, n_last = int((gen[i] >= 0).sum()), int((last[i] >= 0).sum())
        assert n_last >= 1 and np.array_equal(gen[i, n_gen - n_last:n_gen], last[i, :n_last])     # the last step's tokens end the sequence
        root = [k for k in range(rows.shape[0]) if rows[k, 0] == i and rows[k, 1] == 0]
        assert len(root) == 1 and int(np.argmax(lg[root[0]])) == int(last[i, 0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_full_adds_the_rest_on_the_same_timed_steps(tmp_path):
    """Without --full a run prints one line (no BENCH_DETAIL record) and measures nothing beyond its timed steps: no native-loop
    or fixed-tree legs, no bs=1 roofline profile, no CPU leg, no secondary legs.  --full adds them after the timed region, so the
    timed steps of both runs compute the same: equal dumps, accept lengths and headline fields."""
    def run(out_dir, *extra):
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--layers', '2',
               '--dump-outputs', str(out_dir)] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
        out = [ln for ln in r.stdout.splitlines() if ln.startswith(('{', 'BENCH_DETAIL'))]      # (the runtime may print notices)
        assert out and out[-1].startswith('{"metric"') and sum(ln.startswith('{"metric"') for ln in out) == 1, out
        names = ('generated_tokens', 'last_step_tokens', 'last_step_logits', 'last_step_logit_rows')
        return out, json.loads(out[-1]), {n: np.load(os.path.join(out_dir, n + '.npy')) for n in names}
    out_p, plain, dump_p = run(tmp_path / 'plain')
    assert len(out_p) == 1, out_p                                # no BENCH_DETAIL record
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in plain
    assert plain['steps'] == 3 and plain['warmup'] == 1 and plain['config']['lookahead_equals_greedy'] is True
    assert plain['roofline'] is None and plain['cpu_baseline'] is None and 'secondary' not in plain
    assert 'native_loop' not in plain['config'] and 'detail' not in plain['notes'] and 'workload' in plain['notes']
    out_f, full, dump_f = run(tmp_path / 'full', '--full', '--no-cpu-baseline', '--secondary', '')
    assert any(ln.startswith('BENCH_DETAIL {') for ln in out_f)
    assert full['roofline']['verify_step']['ms_graph_step'] > 0 and full['config']['native_loop']['equals_greedy'] is True
    detail = json.loads([ln for ln in out_f if ln.startswith('BENCH_DETAIL {')][0][len('BENCH_DETAIL '):])
    assert all(v['accepted_as_designed'] for v in detail['config']['fixed_tree_sweep'].values())
    for k in ('mean_accept_len', 'mean_draft_len', 'context_mean_timed', 'context_at_end', 'lookahead_equals_greedy'):
        assert plain['config'][k] == full['config'][k], k
    for n in dump_p:
        assert np.array_equal(dump_p[n], dump_f[n]), n
