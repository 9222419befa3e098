"""Host side of the append on the paged KV cache: KVCacheManager.extend against hand-written tables, the runtime key
GenerationSession adds for a paged engine, and the argument checks, which are the linear path's."""
import numpy as np
import pytest

from tensorrt_llm.runtime.generation import GenerationSession, ModelConfig
from tensorrt_llm.runtime.kv_cache_manager import GenerationSequence, KVCacheManager

T, BLOCKS, MAXB = 4, 8, 4
BLOCK_ELEMS = 2 * T * 8  # [Hkv 2, T, Dh 8]


def manager(blocks=BLOCKS, max_blocks=MAXB, contexts=(0, 0)):
    pool = np.zeros(2 * blocks * BLOCK_ELEMS, np.float16)
    m = KVCacheManager([pool], blocks, T, max_blocks)
    for b, n in enumerate(contexts):
        m.add_sequence(GenerationSequence(b, b), n)
    return m, pool.ctypes.data, BLOCK_ELEMS * 2


def table_of(ids_per_seq, base, nbytes, blocks=BLOCKS, max_blocks=MAXB):
    """the table written out by hand: K pointer base + id * nbytes, V pointer `blocks` blocks further on, 0 where unmapped"""
    t = np.zeros((len(ids_per_seq), 1, 2, max_blocks), np.int64)
    for b, ids in enumerate(ids_per_seq):
        for j, i in enumerate(ids):
            t[b, 0, 0, j] = base + i * nbytes
            t[b, 0, 1, j] = base + (blocks + i) * nbytes
    return t


def test_extend_grows_by_zero_one_and_several_blocks():
    m, base, nbytes = manager()
    # add_sequence(., 0) maps one block each: ids 0 and 1
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), table_of([[0], [1]], base, nbytes))
    m.extend([3, 4])  # 3 and 4 tokens of T = 4: the block each holds is enough (growth by 0, an end on a block's last row)
    assert m.lens == [3, 4]
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), table_of([[0], [1]], base, nbytes))
    m.extend([2, 0])  # 5 tokens: one more block for sequence 0; sequence 1 sits the call out and keeps its row
    assert m.lens == [5, 4]
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), table_of([[0, 2], [1]], base, nbytes))
    m.extend([0, 9])  # 13 tokens: three more blocks for sequence 1, in the order the free list hands them out
    assert m.lens == [5, 13]
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), table_of([[0, 2], [1, 3, 4, 5]], base, nbytes))
    assert m.blocks_manager.num_free_blocks() == 2


def test_extend_interleaves_with_step_and_never_releases():
    m, base, nbytes = manager(contexts=(3, 0))
    m.step([False, False])  # 3 -> 4: token 4 opens a block for sequence 0
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), table_of([[0, 2], [1]], base, nbytes))
    m.extend([1, 1])  # 5 and 2 tokens: both covered
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), table_of([[0, 2], [1]], base, nbytes))
    assert m.lens == [5, 2]


def test_extend_raises_when_the_pool_is_exhausted_and_changes_nothing():
    m, base, nbytes = manager(blocks=4)
    before = m.blocks_manager.get_pointer_array(0).copy()
    with pytest.raises(RuntimeError, match="Can't allocate"):
        m.extend([8, 9])  # one and two more blocks: one more than the two that are free
    assert m.lens == [0, 0] and m.blocks_manager.num_free_blocks() == 2
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), before)
    m.extend([8, 4])  # what fits is served afterwards
    np.testing.assert_array_equal(m.blocks_manager.get_pointer_array(0), table_of([[0, 2], [1]], base, nbytes, blocks=4))
    with pytest.raises(RuntimeError, match='max_blocks_per_seq'):
        manager(max_blocks=2)[0].extend([9, 0])


def test_extend_checks_its_argument():
    m, _, _ = manager()
    with pytest.raises(ValueError, match='one entry per live sequence'):
        m.extend([1])
    with pytest.raises(ValueError, match='negative'):
        m.extend([1, -1])
    assert m.lens == [0, 0]


def test_generation_session_adds_the_runtime_key_for_a_paged_engine_only():
    mc = dict(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64)
    assert GenerationSession._runtime_keys(ModelConfig(paged_kv_cache=True, **mc)) == {'paged_append': 1}
    assert GenerationSession._runtime_keys(ModelConfig(**mc)) == {}


class _Runtime:
    """what append() reaches when nothing refuses the call"""

    def __init__(self):
        self.appended = []

    def append(self, *a):
        self.appended.append(a)

    def logits(self):
        return np.zeros((2, 128), np.float32)


def front_end(paged, tp_size=1):
    from tensorrt_llm import Mapping
    s = GenerationSession.__new__(GenerationSession)
    s._model_config = ModelConfig(vocab_size=128, num_layers=2, num_heads=2, hidden_size=64, paged_kv_cache=paged)
    s.mapping = Mapping(tp_size, 0)
    s.batch_size, s.max_input_length, s.max_new_tokens, s.beam_width = 2, 8, 8, 1
    s.runtime = _Runtime()
    return s


@pytest.mark.parametrize('paged', [False, True])
def test_append_argument_checks_are_the_linear_paths(paged):
    s = front_end(paged)
    ok = np.full((2, 3), 5, np.int32)
    s.append(ok)  # a paged engine is no reason to refuse
    s.append(ok, np.array([3, 1]))
    assert len(s.runtime.appended) == 2 and len(s.runtime.appended[1]) == 2
    for bad, lens, err in ((ok[:1], None, ValueError), (ok.astype(np.float32), None, TypeError),
                           (np.full((2, 9), 5, np.int32), None, ValueError), (np.full((2, 2), 128, np.int32), None, ValueError),
                           (ok[0], None, ValueError), (ok, np.array([3, 0]), ValueError), (ok, np.array([4, 1]), ValueError)):
        with pytest.raises(err):
            s.append(bad, lens)
    assert len(s.runtime.appended) == 2
    s.beam_width = 2
    with pytest.raises(ValueError, match='beam_width 1'):
        s.append(ok)


@pytest.mark.parametrize('paged', [False, True])
def test_tensor_parallelism_is_what_append_still_refuses(paged):
    with pytest.raises(NotImplementedError, match='tensor parallelism') as e:
        front_end(paged, tp_size=2).append(np.full((2, 3), 5, np.int32))
    assert 'paged' not in str(e.value)
