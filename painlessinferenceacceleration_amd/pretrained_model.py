# -*- coding: utf-8 -*-
"""lookahead_generation() on the MI355X engine — same entry point, arguments and outputs as
LookaheadPreTrainedModel.lookahead_generation (lookahead/lookahead/common/pretrained_model.py:947-1268).

Per verify step the host does exactly three things: one native trie query (la_cache_hier_get), one
la_llama_step (h2d of ids + 64-bit row masks, the captured graph: forward, accept scan, KV commit; d2h of the
accepted tokens) and one native trie update (la_cache_stream_put).  The reference's >= 15 host<->device
synchronisations per step become one.
"""
import time
from threading import Thread

import numpy as np
import torch

from . import _lib
from .lookahead_generation_utils import (LookaheadDecoderOnlyOutput, _custom_stop, _max_length_of, _parents_of,  # noqa: F401
                                          begin_request, device_stages, gc_paused, pick_token, plan_device_stages, plan_logprobs,
                                          plan_top_logprobs, read_top_logprobs,
                                          run_generate)

_ONE = np.array([1], dtype=np.uint64)


def _pack_rows(mask, W=None):
    """0/1 mask [T][T] -> packed ancestor rows: uint64[T] (T <= 64) or uint64[T][W] (word w = columns 64 w .. 64 w + 63)."""
    m = np.asarray(mask).astype(np.uint64)
    T = m.shape[1]
    W = (T + 63) // 64 if W is None else W
    out = np.zeros((m.shape[0], W), dtype=np.uint64)
    for w in range(W):
        cols = m[:, 64 * w:64 * w + 64]
        if cols.shape[1]:
            out[:, w] = (cols << np.arange(cols.shape[1], dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64)
    return out[:, 0] if W == 1 else out


class LookaheadPreTrainedModel(object):
    """Mixin over an object that owns `self.engine` (LlamaVerifyEngine) and optionally `self.lookahead_cache`."""

    engine = None
    generation_config = None

    # ---------------------------------------------------------------------------------------- draft retrieval
    def lookahead_prepare_inputs_for_generation(self, tail_ids, decoding_kwargs, seq_len):
        """pretrained_model.py:666-756, decode branch: query the trie with the last `max_query_length` tokens.
        Returns (ids int32[T], rowmask uint64[T]) — the rank-4 mask is never materialised (a13/a14)."""
        decoding_length = decoding_kwargs.get('decoding_length', 64)
        branch_length = decoding_kwargs.get('branch_length', 12)
        decoding_mode = decoding_kwargs.get('decoding_mode', 'hier')
        max_length = decoding_kwargs.get('max_length', 2048)
        max_query_length = decoding_kwargs.get('max_query_length', 2)
        update_branch_length = min(branch_length, max_length - seq_len - 1)
        assert update_branch_length >= 0, f'{branch_length=} {max_length=} {seq_len=} {update_branch_length=}'
        qids = tail_ids[-max_query_length:]
        if decoding_mode in ('hier', 'par', 'one'):
            decoding_mode = decoding_mode + '_mix'
        fmt, mode = decoding_mode.split('_')
        tidx = int(decoding_kwargs.get('_trie_idx', 0))      # input-frequency plane: 0, or the global batch index of a sharded job
        ts = time.time()
        if fmt == 'hier' and decoding_kwargs.get('device_trie', False) and len(qids) <= 8 and decoding_length <= _lib.LA_TREE_WIDE_MAX:
            # draft from the workgroup-per-query trie walk over the incremental device mirror (csrc/la_trie_wg.hip; trees wider than one
            # 64-row block come back with uint64[T][4] row masks): bit-identical to the host query; opt-in here because one host query
            # (~20 us) is faster than sync + launch + D2H at bs = 1
            got = self._device_trie().hier_get([list(qids)], decoding_length=decoding_length, branch_length=update_branch_length,
                                               min_input_size=0, min_output_size=max(decoding_length // 2, 1), mode=mode, idxs=[0])[0]
            ids, rowmask, sizes = np.asarray(got[0], dtype=np.int32), np.asarray(got[1], dtype=np.uint64), got[2]
        elif fmt == 'one' and decoding_kwargs.get('device_trie', False) and len(qids) <= 8 and update_branch_length < 64:
            got = self._device_trie(narrow=True).one_get([list(qids)], decoding_length=decoding_length, branch_length=update_branch_length,
                                              mode=mode, idxs=[0])[0]
            ids, rowmask, sizes = np.asarray(got[0], dtype=np.int32), np.asarray(got[1], dtype=np.uint64), got[2]
        elif fmt == 'par' and decoding_kwargs.get('device_trie', False) and len(qids) <= 8 and decoding_length <= 64:
            # par = the hierarchical draft re-laid as independent chains (lookahead_cache.py:441-488): the device retrieves, the
            # re-layout (a handful of set operations on <= 64 rows) stays on the host
            got = self._device_trie(narrow=True).hier_get([list(qids)], decoding_length=decoding_length, branch_length=update_branch_length,
                                                          min_input_size=0, min_output_size=max(decoding_length // 2, 1), mode=mode, idxs=[0])[0]
            T0 = len(got[0])
            dense = np.array([[(int(got[1][i]) >> j) & 1 for j in range(T0)] for i in range(T0)], dtype=np.int64).reshape(T0, T0)
            lst, mask, sizes = self.lookahead_cache.par_layout(got[0], dense)
            ids = np.asarray(lst, dtype=np.int32)
            rowmask = _pack_rows(mask, None)
        elif fmt == 'hier':
            ids, rowmask, _, sizes = self.lookahead_cache.hier_get_packed(
                qids, decoding_length=decoding_length, branch_length=update_branch_length, min_input_size=0,
                min_output_size=max(decoding_length // 2, 1), mode=mode, idx=tidx)
        else:
            lst, mask, sizes = getattr(self.lookahead_cache, fmt + '_get')(
                qids, decoding_length=decoding_length, branch_length=update_branch_length, min_input_size=0,
                min_output_size=max(decoding_length // 2, 1), mode=mode, idx=tidx)
            ids = np.asarray(lst, dtype=np.int32)
            rowmask = _pack_rows(mask, (decoding_length + 63) // 64 if decoding_length > 64 and len(lst) > 1 else None)
        decoding_kwargs['qts'].append(time.time() - ts)
        decoding_kwargs.update({'decoding_qids': qids, 'decoding_ids': ids, 'sizes': sizes})
        return ids, rowmask

    def _device_trie(self, narrow=False):
        """DeviceTrie over self.lookahead_cache, input-frequency plane of idx 0 (rebuilt when the cache object changes; narrow: also when
        its result block grew to 256 rows per query — the one-branch walk writes 64-row blocks)."""
        from .device_trie import DeviceTrie
        dt = getattr(self, '_dev_trie', None)
        if dt is None or dt.cache is not self.lookahead_cache or dt._revoked or (narrow and dt.rows != 64):        # another DeviceTrie took the cache's mirror
            dt = self._dev_trie = DeviceTrie(self.lookahead_cache, idxs=[0], device=self.engine.device)
        return dt

    # ---------------------------------------------------------------------------------------------- the loop
    @torch.no_grad()
    def lookahead_generation(self, *args, **kwargs):
        """Entry point (signature of the reference's lookahead_generation, see _lookahead_generation); the step loop runs with
        the cyclic garbage collector paused (gc_paused)."""
        with gc_paused():
            return self._lookahead_generation(*args, **kwargs)

    def _lookahead_generation(self, input_ids, logits_processor=None, stopping_criteria=None, max_length=None,
                             pad_token_id=None, eos_token_id=None, output_attentions=None,
                             output_hidden_states=None, output_scores=None, return_dict_in_generate=None,
                             synced_gpus=False, streamer=None, **model_kwargs):
        # processors are applied sequentially along the accepted path (pretrained_model.py:834), so a non-empty
        # list (or sampling) takes the host-walked path: device forward only (mode 2), one logits row per accepted token,
        # host-decided commit.  The empty-list greedy default stays entirely on the device.
        # `scores` as the reference returns them (pretrained_model.py:1092, 1195, 1208-1209): ONE entry per verify step, and that entry
        # is model_kwargs['next_tokens_scores'] — which only the no-draft branch writes (:795: the prefill and steps whose retrieval
        # came back empty).  A step WITH drafts therefore appends the previous no-draft step's tensor again (pinned on
        # tests/golden/llama_tiny_scores_fp32.npz).  decoding_kwargs['fresh_scores'] = True (an extension) appends, on draft steps,
        # the processed logits row the step's LAST emitted token was picked from instead.
        logits_processor, sequential, pad_token_id, eos_token_id, return_dict_in_generate, scores, decoding_kwargs, stop_max_length = \
            begin_request(self, logits_processor, stopping_criteria, max_length, pad_token_id, eos_token_id, output_attentions,
                          output_hidden_states, output_scores, return_dict_in_generate, model_kwargs)
        decoding_kwargs['eos'] = eos_token_id[0] if eos_token_id is not None else 2
        decoding_length = decoding_kwargs.get('decoding_length', 64)
        # trees wider than one 64-row block run as consecutive blocks of one multi-block pass (eng.tstep; the reference's best
        # published setting is decoding_length=128, branch_length=32, lookahead/README.md:100)
        wide = int(decoding_length) > _lib.LA_TREE_MAX
        if not 1 <= int(decoding_length) <= _lib.LA_TREE_WIDE_MAX:
            raise ValueError(f'decoding_length={decoding_length}: a draft tree holds at most {_lib.LA_TREE_WIDE_MAX} tokens '
                             f'(4 blocks of 64 rows; the reference grid-searches up to 256, benchmarks/benchmark.py:358)')
        if wide and 64 * int(getattr(self.engine, 'max_blocks', 0) or 0) < int(decoding_length):
            raise ValueError(f'decoding_length={decoding_length} needs an engine created with max_blocks >= '
                             f'{(int(decoding_length) + 63) // 64} (LlamaForCausalLM(..., max_blocks=...))')
        if int(decoding_kwargs.get('branch_length', 12)) + 1 > (_lib.LA_MOUT_TOKS if wide else 64):
            raise ValueError(f'branch_length={decoding_kwargs.get("branch_length")}: a step emits at most {_lib.LA_MOUT_TOKS} tokens')
        if int(decoding_kwargs.get('max_query_length', 2)) < 1:
            raise ValueError('max_query_length must be >= 1')
        decoding_kwargs['max_length'] = stop_max_length
        decoding_kwargs['decoding_max_length'] = stop_max_length + decoding_length + 1
        attention_mask = model_kwargs.get('attention_mask', None)
        if attention_mask is not None and attention_mask.dim() == 2 and not bool(attention_mask.bool().all()):
            raise NotImplementedError('left-padded prompts need the batch path (bs=1 engine assumes no padding)')

        assert input_ids.size(0) == 1
        out_device = input_ids.device
        seq = input_ids[0].tolist()
        n_prompt = len(seq)
        branch_length = decoding_kwargs.get('branch_length', 12)
        eng = self.engine
        # a list that is exactly one RepetitionPenaltyLogitsProcessor runs as a stage of the device step (the penalised argmax of
        # every tree row, then the fused accept walk: csrc/la_penalty.hip) and keeps the graph, the fused tail and the native loop;
        # every other list, sampling, scores, wide trees, the device trie and sharded jobs keep the host walk below
        # a do_sample request that names decoding_kwargs['sample_seed'] and whose list is [repetition penalty?] + [temperature?,
        # top-k?, top-p?] runs as the sampling stage of the device step (csrc/la_sample.hip: the seeded draw of every tree row,
        # then the same accept walk) under the same conditions; without the key it takes the host walk exactly as before
        do_sample = bool(decoding_kwargs.get('do_sample', False))
        stages = plan_device_stages(logits_processor, eng, sequential and scores is None and not wide
                                    and decoding_kwargs.get('gather', None) is None and not decoding_kwargs.get('device_trie', False),
                                    do_sample=do_sample, seed=decoding_kwargs.get('sample_seed', None),
                                    enabled=decoding_kwargs.get('device_processors', True))
        if stages is not None:
            sequential = False
        # decoding_kwargs['output_logprobs']: the log-probability stage of the device step (csrc/la_logprob.hip) — honoured whenever
        # the request runs the device accept, refused (before any engine or trie call) when it would take the host walk
        # decoding_kwargs['top_logprobs'] = n: + the n most likely tokens of every generated position (implies output_logprobs)
        top_n = plan_top_logprobs(decoding_kwargs.get('top_logprobs', 0), eng)
        want_logprobs = plan_logprobs(decoding_kwargs.get('output_logprobs', False) or top_n > 0, eng, sequential,
                                      do_sample=do_sample, seed=decoding_kwargs.get('sample_seed', None),
                                      enabled=decoding_kwargs.get('device_processors', True),
                                      scores=scores is not None or bool(decoding_kwargs.get('fresh_scores', False)), wide=wide,
                                      device_trie=bool(decoding_kwargs.get('device_trie', False)),
                                      gather=decoding_kwargs.get('gather', None) is not None)
        logprobs = top_logprobs = None
        cap = eng._capacity() if hasattr(eng, '_capacity') else eng.max_keys
        assert stop_max_length + decoding_length + 1 <= cap, f'engine KV capacity {cap} < max_length + decoding_length + 1'
        # Sharded job (distributed.py): decoding_kwargs['gather'] = AcceptedTokenGather(..., b_loc=1, mode='strict' | 'split-phase').
        # This rank decodes ITS sequence; every trie call is keyed by the sequence's GLOBAL batch index, the per-step stream_put
        # becomes the all-gather of all ranks' accepted tokens applied in batch-index order (pretrained_model_batch.py:1254-1259),
        # and the rank keeps serving the collective after its own sequence has finished.
        gather = decoding_kwargs.get('gather', None)
        if gather is not None:
            assert gather.b_loc == 1, 'one sequence per rank on this loop (pretrained_model_batch.py takes B_loc > 1)'
            assert not decoding_kwargs.get('device_trie', False), 'sharded decoding keeps the trie replicas on the host'
        tidx = gather.global_index(0) if gather is not None else 0
        decoding_kwargs['_trie_idx'] = tidx
        if gather is not None:
            gather.begin_request()         # no state of an earlier request (un-collected gather, all_done) leaks into this one
        if gather is not None:            # every replica holds every sequence's input frequencies, put in batch-index order
            for b_, p_ in enumerate(gather.exchange_prompts([seq[1:]])):
                self.lookahead_cache.put(p_, branch_length=branch_length + 1, mode='input', idx=b_)
        else:
            self.lookahead_cache.put(seq[1:], branch_length=branch_length + 1, mode='input', idx=0)
        ts = time.time()
        eng.reset()
        first = True
        eos_set = set(eos_token_id) if eos_token_id is not None else set()
        dm = decoding_kwargs.get('decoding_mode', 'hier')
        dm = dm + '_mix' if dm in ('hier', 'par', 'one') else dm
        native_mode = {'input': 0, 'output': 1, 'mix': 2}.get(dm.split('_')[1], 2)
        max_query_length = int(decoding_kwargs.get('max_query_length', 2))
        custom_stop = _custom_stop(stopping_criteria)      # user StoppingCriteria: evaluated per step, interpreter loop only
        fresh_scores = scores is not None and bool(decoding_kwargs.get('fresh_scores', False))
        if fresh_scores:
            sequential = True            # the host walk sees every logits row it picks from
        native_loop = (not sequential and streamer is None and dm.split('_')[0] == 'hier' and not wide
                       and custom_stop is None and gather is None and scores is None
                       and not decoding_kwargs.get('device_trie', False)
                       and not decoding_kwargs.get('debug_lookahead', False) and decoding_kwargs.get('native_loop', True)
                       and 1 <= max_query_length <= 8          # la_lookahead_decode's query buffer; longer queries use this loop
                       and len([e for e in (eos_token_id or []) if e is not None]) <= 8      # ... and its eos list (la_decode_params.eos[8])
                       and hasattr(eng, 'decode_native'))

        def pick(scores_ids, row):
            lg = eng.mlogits() if wide else eng.logits()
            tok, sc = pick_token(logits_processor, do_sample, scores_ids, lg[row], eng.device)
            if scores is not None:
                picked[0] = sc.clone()
            return tok

        picked = [None]            # scores of the last pick() call
        last_scores = None         # what the reference's model_kwargs['next_tokens_scores'] holds
        flushed = False
        try:
            with device_stages(eng, stages, [(0, 0, None)], logprobs=want_logprobs, **({'top_logprobs': top_n} if top_n else {})):      # (row None: prefill seeds the penalty context with the prompt)
                while True:
                    if first:
                        host_row = sequential or scores is not None      # the last prompt row's logits must stay readable
                        if wide:
                            tok = eng.mprefill(0, seq)
                            row = (len(seq) - 1) % (64 * eng.max_blocks)
                        else:
                            tok = eng.prefill(seq, fast=False) if host_row else eng.prefill(seq)
                            row = (len(seq) - 1) % 64
                        if host_row:
                            t = pick(seq, row)                           # sequential: THE pick; otherwise the same argmax, taken for its scores
                            next_tokens = [t] if sequential else [tok]
                        else:
                            next_tokens = [tok]
                        last_scores = picked[0]
                        decoding_kwargs['dls'].append(1)
                        decoding_kwargs['edls'].append(1)
                        first = False
                    else:
                        ids, rowmask = self.lookahead_prepare_inputs_for_generation(seq, decoding_kwargs, len(seq))
                        if len(ids) == 0:
                            ids, rowmask = np.asarray(seq[-1:], dtype=np.int32), _ONE
                        if sequential:
                            T = len(ids)
                            if wide:
                                eng.tstep(ids, rowmask, mode=2)
                            else:
                                eng.verify_only(ids, rowmask)
                            parent = _parents_of(rowmask, T)
                            # every row whose parent is live and whose token was picked stays live; the first one supplies the
                            # next logits row (the reference's surviving leaf branches, pretrained_model.py:831, 850-860: in a
                            # par layout a shared prefix is duplicated across chains and the walk may move to a later chain)
                            cur, live, rows, next_tokens = 0, {0}, [0], []
                            while True:
                                t = pick(seq + next_tokens, cur)
                                next_tokens.append(t)
                                nxt = [j for j in range(1, T) if parent[j] in live and int(ids[j]) == t]
                                if not nxt:
                                    break
                                cur, live = nxt[0], set(nxt)
                                rows.append(cur)
                            if wide:
                                eng.tcommit(rows, T)
                            else:
                                eng.commit(rows)
                        elif wide:
                            next_tokens, _ = eng.tstep(ids, rowmask, mode=0)
                        elif gather is not None and hasattr(eng, 'step_async'):
                            eng.step_async(ids, rowmask, mode=0)
                            gather.overlap(self.lookahead_cache, branch_length)      # split-phase: the previous step's gather + puts, under this pass
                            next_tokens, _ = eng.step_finish()
                        else:
                            next_tokens, _ = eng.step(ids, rowmask, mode=0)
                        if scores is not None:
                            if sequential:
                                if len(ids) <= 1 or fresh_scores:        # no-draft step (:783-795) — or every step (extension)
                                    last_scores = picked[0]
                            elif len(ids) <= 1:
                                # device-accepted step without drafts: the block's only logits row, through the (empty) processor list
                                lg = eng.mlogits() if wide else eng.logits()
                                last_scores = lg[0][None].clone()
                        decoding_kwargs['dls'].append(len(ids))
                        decoding_kwargs['edls'].append(len(next_tokens))
                        if decoding_kwargs.get('debug_lookahead', False):
                            tok = decoding_kwargs.get('tokenizer', None)
                            words = '' if tok is None else tok.decode(next_tokens)
                            print(f'decoding_length:{len(ids)} accept_length:{len(next_tokens)} '
                                  f'query:{decoding_kwargs["decoding_qids"]} hits:{decoding_kwargs["sizes"]} '
                                  f'accept_token:{next_tokens} accept_word:{words}')
                    seq.extend(next_tokens)
                    if scores is not None:
                        scores += (last_scores,)
                    if streamer is not None:
                        streamer.put(np.array([next_tokens]))
                    finished = len(seq) >= stop_max_length or any(t in eos_set for t in next_tokens) or \
                        (custom_stop is not None and custom_stop(seq, out_device, scores))           # :1225-1231
                    if gather is not None:
                        gather.step_update(self.lookahead_cache, next_tokens, branch_length, done=finished)
                    else:
                        self.lookahead_cache.stream_put(next_tokens, branch_length=branch_length + 1, final=False,
                                                        mode='output', idx=0)
                    te = time.time()
                    decoding_kwargs['fts'].append(te - ts)
                    ts = te
                    if finished:
                        if gather is not None:
                            gather.drain(self.lookahead_cache, branch_length)          # until every rank's sequence has finished
                            gather.flush(self.lookahead_cache, branch_length)
                        else:
                            self.lookahead_cache.stream_put([], branch_length=branch_length + 1, final=True, mode='output', idx=0)
                        flushed = True
                        break
                    if native_loop:
                        # every remaining step runs in la_lookahead_decode: same calls in the same order (hier_get -> la_llama_step
                        # -> stream_put -> stop checks), without the interpreter between them
                        new, dls_, edls_, fts_, qts_, fin = eng.decode_native(
                            self.lookahead_cache, seq, stop_max_length, eos_ids=eos_set, decoding_length=decoding_length,
                            branch_length=branch_length, max_query_length=decoding_kwargs.get('max_query_length', 2),
                            mode=native_mode, idx=0)
                        seq.extend(new)
                        decoding_kwargs['dls'].extend(dls_)
                        decoding_kwargs['edls'].extend(edls_)
                        decoding_kwargs['fts'].extend(fts_)
                        decoding_kwargs['qts'].extend(qts_)
                        assert fin
                        self.lookahead_cache.stream_put([], branch_length=branch_length + 1, final=True, mode='output', idx=0)
                        flushed = True
                        break
                if want_logprobs:          # read once: the steps kept the position-indexed log current on the device
                    logprobs = [float(x) for x in eng.logprobs(0, n_prompt, len(seq) - n_prompt)]
                    if top_n:
                        top_logprobs = read_top_logprobs(eng, 0, n_prompt, len(seq) - n_prompt)
        finally:
            # an exception mid-generation must not leave this request's stream buffer / input frequencies behind (they would
            # mix into the next request); the reference flushes on the normal path only (pretrained_model.py:1236-1239)
            if not flushed:
                if gather is not None:
                    # sharded request: this rank failed (or was interrupted) mid-request — it must still serve the per-step collective
                    # until every rank has finished, and flush ALL B sequences, or the other ranks would block in drain() / finish() and
                    # this replica would keep un-flushed stream buffers of the other sequences (AcceptedTokenGather.abort_request)
                    gather.abort_request(self.lookahead_cache, branch_length)
                else:
                    self.lookahead_cache.stream_put([], branch_length=branch_length + 1, final=True, mode='output', idx=tidx)
        if streamer is not None:
            streamer.end()
        sequences = torch.tensor([seq], dtype=torch.long, device=out_device)
        if return_dict_in_generate:
            kwargs = {k: decoding_kwargs[k] for k in ('dls', 'edls', 'fts', 'qts')}
            if want_logprobs:
                kwargs['logprobs'] = logprobs
            if top_n:
                kwargs['top_logprobs'] = top_logprobs
            if scores is not None:
                scores = tuple(s_.to(out_device) for s_ in scores)
            return LookaheadDecoderOnlyOutput(sequences=sequences, scores=scores, attentions=None, hidden_states=None,
                                              kwargs=kwargs)
        return sequences

    # ---------------------------------------------------------------------------------- plain greedy (mode off)
    @torch.no_grad()
    def greedy_search(self, input_ids, max_length, eos_token_id=None, logits_processor=None, do_sample=False,
                      stopping_criteria=None, device_processors=True, sample_seed=None, output_logprobs=False, top_logprobs=0):
        """Plain decoding through the same engine (T=1 blocks): the `use_lookahead=False` leg of the reference's
        examples (examples/llama_example.py:39-69).  With a processor list or sampling each token is picked on the host
        from the block's logits row (forward-only step + commit) — except a list that is exactly one repetition penalty, or a
        do_sample request with an int `sample_seed` whose list device_sampling accepts, which run as the device stages
        lookahead_generation uses (device_processors=False: the host pick).  With the same seed this is the no-draft comparator of
        the sampling lookahead loop: token for token the same sequence.  output_logprobs=True: -> (sequences, list of one
        log-probability per generated token) from the device stage lookahead_generation uses — its no-draft comparator; a request
        that would pick on the host is refused (ValueError).  top_logprobs=n (implies output_logprobs): -> (sequences, logprobs, per
        generated token a list of the n most likely (token_id, logprob) pairs) from the top-N stage."""
        eos = set([eos_token_id] if isinstance(eos_token_id, int) else (eos_token_id or []))
        seq = input_ids[0].tolist()
        n_prompt = len(seq)
        eng = self.engine
        host_pick = do_sample or (logits_processor is not None and len(logits_processor) > 0)
        stages = plan_device_stages(logits_processor, eng, host_pick, do_sample=do_sample, seed=sample_seed, enabled=device_processors)
        if stages is not None:
            host_pick = False
        top_n = plan_top_logprobs(top_logprobs, eng)
        want_logprobs = plan_logprobs(output_logprobs or top_n > 0, eng, host_pick, do_sample=do_sample, seed=sample_seed, enabled=device_processors)
        eng.reset()
        custom_stop = _custom_stop(stopping_criteria)        # the caller's criteria besides the length bound, once per token

        def pick(row):
            return pick_token(logits_processor, do_sample, seq, eng.logits()[row], eng.device)[0]

        with device_stages(eng, stages, [(0, 0, None)], logprobs=want_logprobs, **({'top_logprobs': top_n} if top_n else {})):
            tok = eng.prefill(seq, fast=False) if host_pick else eng.prefill(seq)
            if host_pick:
                tok = pick((len(seq) - 1) % 64)
            seq.append(tok)
            while len(seq) < max_length and tok not in eos and not (custom_stop is not None and custom_stop(seq, input_ids.device)):
                if host_pick:
                    eng.verify_only(np.asarray([tok], dtype=np.int32), _ONE)
                    tok = pick(0)
                    eng.commit([0])
                else:
                    toks, _ = eng.step(np.asarray([tok], dtype=np.int32), _ONE, mode=0)
                    tok = toks[0]
                seq.append(tok)
            if want_logprobs:
                logprobs = [float(x) for x in eng.logprobs(0, n_prompt, len(seq) - n_prompt)]
            if top_n:
                tops = read_top_logprobs(eng, 0, n_prompt, len(seq) - n_prompt)
        sequences = torch.tensor([seq], dtype=torch.long, device=input_ids.device)
        if top_n:
            return sequences, logprobs, tops
        return (sequences, logprobs) if want_logprobs else sequences

    # ------------------------------------------------------------------------------------------- front door
    def generate(self, inputs=None, generation_config=None, logits_processor=None, stopping_criteria=None,
                 prefix_allowed_tokens_fn=None, synced_gpus=None, assistant_model=None, streamer=None, **kwargs):
        """generate() with the reference's signature (common/pretrained_model.py:110-121) for the two modes this package serves —
        lookahead and plain greedy / sampling through the same engine.  Everything the reference derives before it dispatches is
        derived the same way (lookahead_generation_utils.resolve_generate_args): keyword > generation_config > model defaults,
        config-derived logits processors (repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens)
        with the caller's `logits_processor` merged behind them, MaxLengthCriteria / MaxTimeCriteria with the caller's
        `stopping_criteria` merged behind them; the lookahead branch receives processors + criteria and no warper, exactly as
        :428-441; temperature / top_k / top_p act in the sampling mode (`do_sample` without lookahead, :465-479).
        Call shapes of the reference's own callers work unchanged: examples/llama_example.py:51-60,
        benchmarks/benchmark.py:282-300."""
        return run_generate(self, False, inputs, generation_config, logits_processor, stopping_criteria, prefix_allowed_tokens_fn,
                            assistant_model, streamer, kwargs)

    def stream_generate(self, *args, **kwargs):
        """pretrained_model.py:1323-1350: run generate() on a worker thread, yield from the streamer."""
        streamer = kwargs.get('streamer')
        assert streamer is not None, 'stream_generate needs a streamer with an iterator interface'
        Thread(target=self.generate, args=args, kwargs=kwargs).start()
        for item in streamer:
            yield item
