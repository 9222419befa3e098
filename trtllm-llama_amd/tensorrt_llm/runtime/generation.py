"""GenerationSession (T/tensorrt_llm/runtime/generation.py:141-156,413-488,782-997) over the C++ host loop.

Same objects and call sequence as the reference examples use:
    model_config = ModelConfig(num_heads=.., hidden_size=.., vocab_size=.., num_layers=.., gpt_attention_plugin=..)
    sampling_config = SamplingConfig(end_id=2, pad_id=2, num_beams=1)
    decoder = GenerationSession(model_config, engine_buffer, mapping)
    decoder.setup(batch_size, max_input_length, max_new_tokens)
    output_ids = decoder.decode(input_ids, input_lengths, sampling_config)   # int32 [batch, beams, max_in + max_new]
The per-step bookkeeping of the reference's Python loop (sequence_length = max_in + step, past_key_value_length =
[0,1] then [max_in + step, 0], masked_tokens[b, len_b:max_in] = 1, ping-pong contexts, a device->host sync per step:
generation.py:490-699, :812-821, :963) lives on the device inside tllm_session_generate."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from ..mapping import Mapping
from .native import NativeSession


@dataclass
class ModelConfig:
    vocab_size: int
    num_layers: int
    num_heads: int
    hidden_size: int
    gpt_attention_plugin: bool = True
    multi_query_mode: bool = False
    remove_input_padding: bool = False
    model_name: str = ''
    paged_kv_cache: bool = False
    tokens_per_block: int = 64
    use_prompt_tuning: bool = False
    num_kv_heads: int = None  # grouped-query attention: K/V heads of this rank (None: num_heads); the engine header is what the session runs
    lora_max_rank: int = 0  # LoRA: what the engine was built with (build.py --lora_max_rank / --lora_target_modules); load_lora() checks
    lora_target_modules: str = None  # an adapter against them before the session does


@dataclass
class SamplingConfig:
    end_id: int
    pad_id: int
    num_beams: int = field(default=1)
    temperature: float = field(default=1.0)
    top_k: int = field(default=1)
    top_p: float = field(default=0.0)
    length_penalty: float = field(default=1.0)
    repetition_penalty: float = field(default=1.0)
    min_length: int = field(default=1)
    presence_penalty: float = field(default=0.0)
    use_beam_hyps: bool = field(default=True)
    # set after construction, as the reference (generation.py:136); None -> 0 (layers/baseSamplingLayer.cpp:119-123)
    random_seed: int = field(init=False, default=None)


class GenerationSession(object):

    def __init__(self, model_config: ModelConfig, engine_buffer, mapping: Mapping, debug_mode=False):
        assert isinstance(model_config, ModelConfig)
        if not model_config.gpt_attention_plugin:
            raise ValueError('the MI355X LLaMA path needs the gpt_attention plugin (RoPE lives in it)')
        if model_config.multi_query_mode:
            raise NotImplementedError('multi_query_mode is not built')
        self._model_config = model_config
        self.mapping = mapping
        self.debug_mode = debug_mode
        if mapping.tp_size > 1:
            from ..parallel import ensure_tp_communicator
            ensure_tp_communicator(mapping)
        self.runtime = NativeSession(engine=bytes(engine_buffer), runtime_keys=self._runtime_keys(model_config))
        self.runtime.vocab = model_config.vocab_size
        self.batch_size = self.max_input_length = self.max_new_tokens = 0

    @staticmethod
    def _runtime_keys(model_config: ModelConfig) -> dict:
        """Session keys that belong to the runtime and not to the engine header.  paged_append: a paged engine serves append(),
        verify() and decode_lookup() on its block table (the key is refused on a linear cache, so only a paged engine gets it)."""
        return dict(paged_append=1) if model_config.paged_kv_cache else {}

    @property
    def vocab_size(self):
        return self._model_config.vocab_size

    @property
    def num_layers(self):
        return self._model_config.num_layers

    @property
    def num_heads(self):
        return self._model_config.num_heads

    @property
    def num_kv_heads(self):
        """K/V heads of this rank (grouped-query attention); num_heads when the configuration does not say"""
        kv = self._model_config.num_kv_heads
        return self._model_config.num_heads if kv is None else kv

    @property
    def hidden_size(self):
        return self._model_config.hidden_size

    def setup(self, batch_size: int, max_input_length: int, max_new_tokens: int, beam_width: int = 1):
        if not 1 <= beam_width <= 8:
            raise ValueError(f'beam_width {beam_width}: the device-side beam step takes 1 to 8 hypotheses per prompt')
        # batch_size * beam_width sequences: any number; the generation GEMVs take 8 rows per launch, more go through in slabs of 8
        # (each slab streams the weights again - build.py's default --max_batch_size 8 with beam search relies on this)
        self.batch_size, self.max_input_length, self.max_new_tokens = batch_size, max_input_length, max_new_tokens
        self.beam_width = beam_width
        self.runtime.setup(batch_size, max_input_length, max_new_tokens, beam_width)

    def load_lora(self, adapter_dir, slot: int = 0):
        """Load a Hugging Face PEFT LoRA adapter directory (adapter_config.json + adapter_model.safetensors) into adapter slot `slot`
        of an engine built with --lora_max_rank (tensorrt_llm/runtime/lora.py reads it; `peft` is not needed).  Select it per
        sequence with the lora_slots argument of decode() / append() / score() / decode_append() / decode_lookup()."""
        from .lora import load_peft_adapter
        mc = dict(num_layers=self.num_layers)
        if self._model_config.lora_max_rank:
            mc['lora_max_rank'] = self._model_config.lora_max_rank
        if self._model_config.lora_target_modules:
            mc['lora_target_modules'] = self._model_config.lora_target_modules
        ad = load_peft_adapter(adapter_dir, mc)
        self.runtime.lora_load(slot, ad['tensors'], ad['alpha'], use_rslora=ad['use_rslora'])
        return ad

    def _select_lora(self, lora_slots):
        """lora_slots: None (the selection stays what it is: none after setup()) or one adapter slot per sequence, -1 = none"""
        if lora_slots is None:
            return
        slots = np.asarray(lora_slots.cpu() if hasattr(lora_slots, 'cpu') else lora_slots)
        if slots.shape != (self.batch_size, ) or not np.issubdtype(slots.dtype, np.integer):
            raise ValueError(f'lora_slots must be {self.batch_size} integers, one slot per sequence (-1 = no adapter)')
        self.runtime.lora_select(slots.astype(np.int32))

    def decode(self, input_ids, input_lengths, sampling_config: SamplingConfig, prompt_embedding_table=None,
               tasks=None, prompt_vocab_size=None, max_new_tokens: Optional[int] = None, lora_slots=None):
        """input_ids: int32 [batch, max_input_length] (torch tensor or ndarray), padded with pad_id.
        max_new_tokens: fewer than setup()'s (None: all of them) - a first turn that leaves cache room for decode_append().
        Returns int32 [batch, num_beams, max_input_length + max_new_tokens] like the reference (generation.py:991-997):
        num_beams == 1: top-k / top-p sampling with temperature, penalties and min_length on the device (arg-max with the
        default fields), reproducible for a fixed sampling_config.random_seed; beam search (hypotheses best first, back-tracked
        by gather_tree) otherwise."""
        self._check_sampling_config(sampling_config)
        if sampling_config.num_beams != getattr(self, 'beam_width', 1):
            # the reference sizes its beam buffers inside decode() from scfg.num_beams (generation.py:365-411)
            self.setup(self.batch_size, self.max_input_length, self.max_new_tokens, sampling_config.num_beams)
        is_torch = hasattr(input_ids, 'cpu')
        ids = input_ids.cpu().numpy() if is_torch else np.asarray(input_ids)
        lens = input_lengths.cpu().numpy() if hasattr(input_lengths, 'cpu') else np.asarray(input_lengths)
        assert ids.shape == (self.batch_size, self.max_input_length), 'call setup() with matching sizes first'
        if sampling_config.num_beams == 1:
            self.runtime.set_sampling(self._native_sampling(sampling_config))
        new = self.max_new_tokens if max_new_tokens is None else int(max_new_tokens)
        if not 0 <= new <= self.max_new_tokens:
            raise ValueError(f'max_new_tokens {new} outside [0, {self.max_new_tokens}] (setup)')
        self._select_lora(lora_slots)
        out = self.runtime.generate(ids.astype(np.int32), lens.astype(np.int32), new,
                                    end_id=sampling_config.end_id, pad_id=sampling_config.pad_id)
        out = out.reshape(self.batch_size, sampling_config.num_beams, -1)
        if is_torch:
            import torch
            return torch.from_numpy(out).to(input_ids.device)
        return out

    @staticmethod
    def _check_score_args(ids, lens, batch_size: int, max_input_length: int, beam_width: int = 1):
        """What score() refuses before anything reaches the device."""
        if beam_width != 1:
            raise ValueError(f'score() needs beam_width 1 (the session is set up with {beam_width})')
        if ids.ndim != 2 or ids.shape != (batch_size, max_input_length):
            raise ValueError(f'input_ids {ids.shape}: call setup() with matching sizes first '
                             f'(batch {batch_size}, max_input_length {max_input_length})')
        if lens.shape != (batch_size, ):
            raise ValueError(f'input_lengths {lens.shape}: one length per sequence ({batch_size})')
        if not (np.issubdtype(ids.dtype, np.integer) and np.issubdtype(lens.dtype, np.integer)):
            raise TypeError('input_ids and input_lengths must be integers')
        if lens.size and (lens.min() < 1 or lens.max() > max_input_length):
            raise ValueError(f'input_lengths must lie in [1, {max_input_length}]')

    def score(self, input_ids, input_lengths, lora_slots=None):
        """Teacher-forced scoring of the prompts in one prefill (tllm_session_score).  input_ids int32 [batch, max_input_length]
        and input_lengths [batch] as decode() takes them (torch tensor or ndarray).  Returns a dict:
          log_probs  f32 [batch, max_input_length]: log p(ids[b][t] | ids[b][:t]) for 1 <= t < len_b, 0 elsewhere;
          top1_ids   int32, same shape: the arg-max of that distribution, -1 where log_probs is 0 by definition;
          perplexity f32 [batch]: exp(-sum_t log_probs[b][t] / (len_b - 1)); nan for a sequence of one token.
        torch tensors on the input's device when input_ids is a torch tensor.  The session is left as the prompt pass of
        decode() leaves it."""
        from .scoring_ref import perplexity
        is_torch = hasattr(input_ids, 'cpu')
        ids = input_ids.cpu().numpy() if is_torch else np.asarray(input_ids)
        lens = input_lengths.cpu().numpy() if hasattr(input_lengths, 'cpu') else np.asarray(input_lengths)
        self._check_score_args(ids, lens, self.batch_size, self.max_input_length, getattr(self, 'beam_width', 1))
        self._select_lora(lora_slots)
        lp, top = self.runtime.score(ids.astype(np.int32), lens.astype(np.int32))
        ppl = np.array([perplexity(lp[b], lens[b:b + 1]) for b in range(len(lens))], np.float32)
        out = dict(log_probs=lp, top1_ids=top, perplexity=ppl)
        if is_torch:
            import torch
            out = {k: torch.from_numpy(v).to(input_ids.device) for k, v in out.items()}
        return out

    @staticmethod
    def _check_append_args(ids, batch_size: int, max_input_length: int, vocab_size: int, beam_width: int = 1, lengths=None):
        """What append() / decode_append() refuse before anything reaches the device.  lengths (ndarray [batch] or None): tokens
        per sequence in the padded ids [batch, W], each in [1, W]; ids are range-checked below their length only."""
        if beam_width != 1:
            raise ValueError(f'append() needs beam_width 1 (the session is set up with {beam_width})')
        if ids.ndim != 2 or ids.shape[0] != batch_size:
            raise ValueError(f'input_ids {ids.shape}: [batch {batch_size}, n] - the same number of tokens for every sequence')
        if not np.issubdtype(ids.dtype, np.integer):
            raise TypeError('input_ids must be integers')
        if not 1 <= ids.shape[1] <= max_input_length:
            raise ValueError(f'n = {ids.shape[1]} must lie in [1, max_input_length {max_input_length}] '
                             '(longer input: append it in chunks)')
        if lengths is not None:
            if lengths.shape != (batch_size, ):
                raise ValueError(f'input_lengths {lengths.shape}: [batch {batch_size}]')
            if not np.issubdtype(lengths.dtype, np.integer):
                raise TypeError('input_lengths must be integers')
            if lengths.min() < 1 or lengths.max() > ids.shape[1]:
                raise ValueError(f'input_lengths must lie in [1, {ids.shape[1]}] (a sequence cannot sit an append out)')
            ids = ids[np.arange(ids.shape[1])[None, :] < lengths[:, None]]
        if ids.size and (ids.min() < 0 or ids.max() >= vocab_size):
            raise ValueError(f'token ids must lie in [0, {vocab_size})')

    def _append_ids(self, input_ids, input_lengths=None):
        """the checked ids as int32 - and, with input_lengths, (ids, lengths)"""
        ids = input_ids.cpu().numpy() if hasattr(input_ids, 'cpu') else np.asarray(input_ids)
        lens = None
        if input_lengths is not None:
            lens = input_lengths.cpu().numpy() if hasattr(input_lengths, 'cpu') else np.asarray(input_lengths)
        if self.mapping.tp_size > 1:
            raise NotImplementedError('append() is not built for tensor parallelism')
        self._check_append_args(ids, self.batch_size, self.max_input_length, self.vocab_size, getattr(self, 'beam_width', 1), lens)
        if lens is None:
            return ids.astype(np.int32)
        return ids.astype(np.int32), lens.astype(np.int32)

    def append(self, input_ids, input_lengths=None, lora_slots=None):
        """Append input_ids int32 [batch, n] (torch tensor or ndarray; the same n for every sequence, n <= max_input_length) to
        the live KV cache in one prefill pass (tllm_session_append) - the next user turn of a chat, the next chunk of a long
        prompt, n tokens to verify.  Token 0 takes the place of the pending token the last decode() / append() chose (pass that
        token first to keep it).  Returns the fp32 logits [batch, vocab] of the last appended token; the session has chosen
        the next pending token and generation can continue (decode_append, or another append).  Needs a decode() / score()
        before it and room in the cache: setup()'s max_new_tokens bounds everything behind the prompt.
        input_lengths int [batch] (tllm_session_append_ragged): input_ids is padded [batch, W] and sequence b appends its first
        input_lengths[b] ids alone, 1 <= input_lengths[b] <= W; what stands behind them is never read, and the logits of row b are
        those of its own last appended token."""
        self._select_lora(lora_slots)
        if input_lengths is None:
            self.runtime.append(self._append_ids(input_ids))
        else:
            self.runtime.append(*self._append_ids(input_ids, input_lengths))
        logits = self.runtime.logits()
        if hasattr(input_ids, 'cpu'):
            import torch
            return torch.from_numpy(logits).to(input_ids.device)
        return logits

    def decode_append(self, input_ids, sampling_config: SamplingConfig, max_new_tokens: Optional[int] = None, input_lengths=None,
                      lora_slots=None):
        """append(input_ids), then generation as decode() runs it (tllm_session_append_generate), under sampling_config
        (num_beams 1).  max_new_tokens None: as many as the cache still has room for (with input_lengths, as append() takes
        them: the room of the sequence that has the least left; every sequence generates the same number).  Returns int32 [batch, 1, max_input_length
        + max_new_tokens(setup)]: the whole token record - prompt, earlier turns, the appended ids, the new tokens - its unused
        tail filled with end_id (pad_id when end_id < 0)."""
        self._check_sampling_config(sampling_config)
        if sampling_config.num_beams != 1:
            raise ValueError('decode_append() needs num_beams 1')
        lens = None
        if input_lengths is None:
            ids = self._append_ids(input_ids)
        else:
            ids, lens = self._append_ids(input_ids, input_lengths)
        if max_new_tokens is None:
            used = self.runtime.step_state()['sequence_length'] + (ids.shape[1] if lens is None else lens)
            max_new_tokens = self.max_input_length + self.max_new_tokens - int(used.max())
        if max_new_tokens < 1:
            raise ValueError('no room left in the KV cache for a new token: set up with a larger max_new_tokens')
        self.runtime.set_sampling(self._native_sampling(sampling_config))
        self._select_lora(lora_slots)
        out = self.runtime.append_generate(ids, max_new_tokens, end_id=sampling_config.end_id, pad_id=sampling_config.pad_id,
                                           lengths=lens)
        out = out.reshape(self.batch_size, 1, -1)
        if hasattr(input_ids, 'cpu'):
            import torch
            return torch.from_numpy(out).to(input_ids.device)
        return out

    def verify(self, input_ids, sampling_config: Optional[SamplingConfig] = None):
        """Verify input_ids int32 [batch, n] (n <= 32) in one pass over the live cache (tllm_session_verify): token 0 takes the
        pending token's place, the others are drafts of what follows; the longest prefix greedy decoding would have produced is
        kept and the session continues behind it.  Returns a dict: accepted int32 [batch] (drafts kept; -1 for a finished
        sequence), log_probs f32 [batch, n] (log p of every id given what precedes it, 0 for token 0), logits f32 [batch, vocab]
        (the row behind the last kept token).  Without sampling_config: greedy sessions only.
        With a sampling_config (num_beams 1) that is not plain arg-max the session samples under it from here on and the pass is
        tllm_session_verify_sampled's: a draft is kept only where it equals the token the sampler draws there (the token decode()
        would have produced for that configuration and seed); log_probs stay the raw model's."""
        ids = self._append_ids(input_ids)
        sampled = False
        if sampling_config is not None:
            self._check_sampling_config(sampling_config)
            if sampling_config.num_beams != 1:
                raise ValueError('verify() needs num_beams 1')
            self.runtime.set_sampling(self._native_sampling(sampling_config))
            sampled = not self._is_greedy(sampling_config)
        acc, lp = self.runtime.verify(ids, sampled=True) if sampled else self.runtime.verify(ids)
        out = dict(accepted=acc, log_probs=lp, logits=self.runtime.logits())
        if hasattr(input_ids, 'cpu'):
            import torch
            out = {k: torch.from_numpy(v).to(input_ids.device) for k, v in out.items()}
        return out

    @staticmethod
    def _is_greedy(scfg: SamplingConfig) -> bool:
        """plain arg-max, as the device's sampling_is_greedy() decides it"""
        return scfg.top_k == 1 and scfg.temperature == 1.0 and scfg.repetition_penalty == 1.0 and scfg.presence_penalty == 0.0 \
            and scfg.min_length <= 1

    @staticmethod
    def _check_lookup_args(scfg: SamplingConfig, num_draft_tokens: int, max_ngram: int, speculative_sampling: bool = False):
        """What decode_lookup() refuses before anything reaches the device."""
        if scfg.num_beams != 1:
            raise ValueError('decode_lookup() needs num_beams 1')
        if not speculative_sampling and not GenerationSession._is_greedy(scfg):
            raise NotImplementedError('decode_lookup() is greedy: the sampling configuration must be plain arg-max (top_k 1, '
                                      'temperature 1, no penalty, min_length <= 1) - speculative sampling is not built')
        if not 2 <= num_draft_tokens <= 32 or not 1 <= max_ngram <= 8:
            raise ValueError(f'num_draft_tokens {num_draft_tokens} must lie in [2, 32] and max_ngram {max_ngram} in [1, 8]')

    def decode_lookup(self, input_ids, input_lengths, sampling_config: SamplingConfig, num_draft_tokens: int = 8, max_ngram: int = 3,
                      max_new_tokens: Optional[int] = None, speculative_sampling: bool = False, lora_slots=None):
        """decode() with prompt-lookup speculation (tllm_session_generate_lookup): the same tokens, greedy; where the text repeats
        an n-gram of the prompt or of itself, up to num_draft_tokens - 1 following tokens are verified in one pass.  max_new_tokens
        None: setup()'s less num_draft_tokens, the room the last verify pass needs.  Returns what decode() returns; the counters of
        the call are kept in self.lookup_stats (rounds, verify_rounds, step_rounds, drafted, accepted).
        speculative_sampling=True (tllm_session_generate_lookup_sampled) takes any single-beam sampling_config: a draft is kept
        where it equals the token the sampler draws there, so the tokens are decode()'s for that configuration and random_seed."""
        self._check_lookup_args(sampling_config, num_draft_tokens, max_ngram, speculative_sampling)
        if speculative_sampling:
            self._check_sampling_config(sampling_config)
        if getattr(self, 'beam_width', 1) != 1:
            raise ValueError(f'decode_lookup() needs beam_width 1 (the session is set up with {self.beam_width})')
        is_torch = hasattr(input_ids, 'cpu')
        ids = input_ids.cpu().numpy() if is_torch else np.asarray(input_ids)
        lens = input_lengths.cpu().numpy() if hasattr(input_lengths, 'cpu') else np.asarray(input_lengths)
        assert ids.shape == (self.batch_size, self.max_input_length), 'call setup() with matching sizes first'
        new = self.max_new_tokens - num_draft_tokens if max_new_tokens is None else int(max_new_tokens)
        if not 1 <= new <= self.max_new_tokens - num_draft_tokens:
            raise ValueError(f'max_new_tokens {new} outside [1, {self.max_new_tokens - num_draft_tokens}]: setup()\'s less '
                             'num_draft_tokens')
        self.runtime.set_sampling(self._native_sampling(sampling_config))
        self._select_lora(lora_slots)
        out, self.lookup_stats = self.runtime.generate_lookup(ids.astype(np.int32), lens.astype(np.int32), new,
                                                              end_id=sampling_config.end_id, pad_id=sampling_config.pad_id,
                                                              num_draft_tokens=num_draft_tokens, max_ngram=max_ngram,
                                                              **(dict(sampled=True) if speculative_sampling else {}))
        out = out.reshape(self.batch_size, 1, -1)
        if is_torch:
            import torch
            return torch.from_numpy(out).to(input_ids.device)
        return out

    @staticmethod
    def _native_sampling(scfg: SamplingConfig) -> dict:
        return dict(top_k=scfg.top_k, top_p=scfg.top_p, temperature=scfg.temperature,
                    repetition_penalty=scfg.repetition_penalty, presence_penalty=scfg.presence_penalty,
                    min_length=scfg.min_length, random_seed=scfg.random_seed or 0)

    @staticmethod
    def _check_sampling_config(scfg: SamplingConfig):
        """Only what the device-side sampler honours is accepted; a field that would silently change nothing raises
        instead (the reference feeds all of them to DynamicDecodeOp, generation.py:300-345, 949-961).
        num_beams 1: top_k, top_p, temperature, one of repetition_penalty / presence_penalty, min_length and random_seed go
        to the device sampler (csrc/kernels/sampling.hip).
        Beam search: hypotheses are ranked by the raw cumulative log-probability, as the reference's runtime does without
        beam_hyps - so temperature must be 1 and the penalties / min_length, which the beam step does not apply, raise;
        top_k / top_p play no part in the reference's beam search either."""
        if scfg.num_beams == 1:
            if not scfg.temperature > 0:
                raise ValueError('temperature must be positive')
            if scfg.top_k < 0 or not scfg.top_p >= 0:
                raise ValueError('top_k and top_p must not be negative')
            if not scfg.repetition_penalty > 0:
                raise ValueError('repetition_penalty must be positive')
        if scfg.repetition_penalty != 1.0 and scfg.presence_penalty != 0.0:
            # layers/baseSamplingLayer.cpp:149-167
            raise ValueError('repetition_penalty and presence_penalty are mutually exclusive')
        bad = []
        if scfg.num_beams > 1:
            if scfg.repetition_penalty != 1.0:
                bad.append(f'repetition_penalty={scfg.repetition_penalty} with beam search')
            if scfg.presence_penalty != 0.0:
                bad.append(f'presence_penalty={scfg.presence_penalty} with beam search')
            if scfg.min_length > 1:
                bad.append(f'min_length={scfg.min_length} with beam search')
            if scfg.temperature != 1.0:
                bad.append(f'temperature={scfg.temperature} with beam search')
            if scfg.length_penalty != 1.0:
                bad.append(f'length_penalty={scfg.length_penalty}')
        if bad:
            raise NotImplementedError('SamplingConfig fields the device-side sampler does not honour: ' + ', '.join(bad))

    def decode_batch(self, input_ids, sampling_config: SamplingConfig):
        """list of 1-D id tensors -> pads to the longest and decodes (generation.py:770-780)."""
        lens = np.array([len(x) for x in input_ids], np.int32)
        max_len = int(lens.max())
        padded = np.full((len(input_ids), max_len), sampling_config.pad_id, np.int32)
        for i, x in enumerate(input_ids):
            padded[i, :lens[i]] = np.asarray(x.cpu() if hasattr(x, 'cpu') else x)
        return self.decode(padded, lens, sampling_config)
