"""The split-KV plan of the decode attention without a GPU: tllm_attention_decode_layout and tllm_attention_workspace_size
(include/tllm_runtime_api.h) against a plain restatement of the launch rule.  No compute calls.

The rule, with N = 2048 / head_size cache slots per row of a lane group:
  tchunk(rows) = N * rows,  nsplit(rows) = ceil(max_seq_len / tchunk(rows));
  rows_per_group 0: 16 rows while nsplit(16) <= 16 - and 12 while nsplit(12) <= 8 - with the merge inside the launch, else 4 rows
  with the combine launch;  an explicit 4 / 12 / 16: the merge inside the launch iff nsplit <= 16;  combine_launch clears it;
  workspace: the tickets (uint32 per sequence and head), the {max, sum} pairs and the fp32 partial outputs at the FINEST split
  (4 rows), the first two rounded up to 256 bytes, + 256."""
import ctypes
import itertools

import pytest

from tensorrt_llm.plugin import capi


def up256(n):
    return (n + 255) // 256 * 256


def plan(head_size, max_seq_len, batch, num_heads, rows, combine):
    n = 2048 // head_size
    nsplit = lambda r: (max_seq_len + n * r - 1) // (n * r)
    if rows == 0:
        merged = nsplit(16) <= 16
        rows = (12 if nsplit(12) <= 8 else 16) if merged else 4
    else:
        merged = nsplit(rows) <= 16
    bh = batch * num_heads
    workspace = up256(bh * 4) + up256(bh * nsplit(4) * 8) + bh * nsplit(4) * head_size * 4 + 256
    return n * rows, nsplit(rows), int(merged and not combine), workspace


def query(lib, head_size, max_seq_len, batch, num_heads, rows, combine):
    p = capi.AttentionParams(batch=batch, num_heads=num_heads, head_size=head_size, max_seq_len=max_seq_len, rows_per_group=rows,
                             combine_launch=combine)
    a = [ctypes.c_int32(-1) for _ in range(4)]
    rc = lib.tllm_attention_decode_layout(ctypes.byref(p), *[ctypes.byref(x) for x in a])
    return rc, [x.value for x in a], lib.tllm_attention_workspace_size(ctypes.byref(p), 0)


def capacities(head_size):
    n = 2048 // head_size
    return [1, n * 12 * 8, n * 12 * 8 + 1, n * 16 * 16, n * 16 * 16 + 1, n * 4 * 256]


@pytest.mark.parametrize('head_size', [32, 64, 128, 256])
def test_layout_and_workspace_follow_the_rule(lib, head_size):
    for smax, (batch, heads), rows, combine in itertools.product(capacities(head_size), [(1, 2), (3, 8)], [0, 4, 12, 16], [0, 1]):
        what = f'head_size {head_size} max_seq_len {smax} batch {batch} heads {heads} rows_per_group {rows} combine_launch {combine}'
        rc, (tchunk, nsplit, q_tile, merged), workspace = query(lib, head_size, smax, batch, heads, rows, combine)
        assert rc == 0, f'{what}: {capi.last_error()}'
        want = plan(head_size, smax, batch, heads, rows, combine)
        assert (tchunk, nsplit, merged, workspace) == want, what
        assert q_tile == 1, what


def test_the_rule_at_the_bench_shape(lib):
    """The restatement itself, pinned where the numbers are known: head size 128, 16 cache slots per row."""
    assert plan(128, 1536, 1, 32, 0, 0)[:3] == (192, 8, 1)
    assert plan(128, 1537, 1, 32, 0, 0)[:3] == (256, 7, 1)
    assert plan(128, 4096, 1, 32, 0, 0)[:3] == (256, 16, 1)
    assert plan(128, 4097, 1, 32, 0, 0)[:3] == (64, 65, 0)
    assert plan(128, 4097, 1, 32, 16, 0)[:3] == (256, 17, 0)
    assert plan(128, 1024, 1, 32, 4, 1)[:3] == (64, 16, 0)


def test_unsupported_head_size_and_rows_are_refused(lib):
    rc, _, workspace = query(lib, 24, 1024, 1, 2, 0, 0)  # 64 lanes are no multiple of the 3 lanes of a cache row
    assert rc != 0 and 'head_size' in capi.last_error()
    assert workspace == 256  # no plan: nothing but the slack
    rc, _, _ = query(lib, 128, 1024, 1, 2, 5, 0)
    assert rc != 0 and 'rows_per_group' in capi.last_error()
