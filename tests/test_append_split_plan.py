"""tllm_attention_append_split_layout (no GPU): the plan of the split-KV append attention - chunk, ranges, workspace - and its
refusals."""
import pytest

from tensorrt_llm.plugin import capi
from tensorrt_llm.runtime.native import attention_append_split_layout as layout

H, B = 32, 2


@pytest.mark.parametrize('n,Hkv,max_keys,cus', [(1, 32, 0, 256), (2, 32, 1024, 256), (8, 8, 4000, 256), (32, 32, 130, 304),
                                                (15, 1, 65536, 64), (4, 32, 1000000, 256)])
@pytest.mark.parametrize('Dh', [64, 128])
def test_the_plan(n, Hkv, max_keys, cus, Dh):
    for forced in (0, 64, 448):
        chunk, ranges, nbytes = layout(n, Dh, batch=B, num_heads=H, num_kv_heads=Hkv, max_keys=max_keys, cus=cus, split_chunk=forced)
        assert chunk % 64 == 0 and chunk > 0 and (forced == 0 or chunk == forced)
        assert ranges * chunk >= max_keys > (ranges - 1) * chunk
        assert nbytes >= B * n * H * (ranges + 1) * (Dh + 2) * 4
        if forced == 0:  # the rule: at least 128 slots to a range, at most 64 ranges
            assert chunk >= 128 and ranges <= 64


@pytest.mark.parametrize('kw,needle', [(dict(n=2, head_size=32), 'head size'), (dict(n=2, head_size=256), 'head size'),
                                       (dict(n=33, head_size=64), 'n <= 32'), (dict(n=0, head_size=64), 'n <= 32'),
                                       (dict(n=2, head_size=64, split_chunk=96), 'multiple of 64'),
                                       (dict(n=2, head_size=64, split_chunk=-64), 'multiple of 64')])
def test_the_plan_refuses(kw, needle):
    with pytest.raises(RuntimeError, match=needle):
        layout(batch=B, num_heads=H, max_keys=1024, **kw)


def test_the_symbols_are_exported():
    lib = capi.load_library()
    for name in ('tllm_attention_append_split', 'tllm_attention_append_split_layout', 'tllm_session_append_split_launches'):
        assert hasattr(lib, name), name
