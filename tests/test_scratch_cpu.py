"""ops._grow_scratch, the one grow-only scratch pool behind every family's process-wide workspace, on CPU tensors: when it
allocates, when it synchronises, what it keeps.  (What the kernels do with the scratch: test_gpu_workspace.py.)"""
import torch


def test_grow_scratch(monkeypatch):
    from mri_interpolation_amd import ops
    synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: synced.append(device))
    cpu = torch.device("cpu")  # (index None: one slot)
    cache = {}
    # the first call allocates, and nothing can be using a buffer that did not exist
    first = ops._grow_scratch(cache, cpu, 1001)
    assert first.dtype == torch.float32 and first.numel() == 251 and not synced
    assert cache[cpu.index] is first and len(cache) == 1
    # a smaller or equal need: the same tensor
    assert ops._grow_scratch(cache, cpu, 12) is first and ops._grow_scratch(cache, cpu, 1004) is first and not synced
    # a larger need: one synchronisation of that device, then the entry is replaced
    second = ops._grow_scratch(cache, cpu, 1005)
    assert second is not first and second.numel() == 252 and synced == [cpu]
    assert cache[cpu.index] is second and len(cache) == 1
    # nothing needed: what is cached
    assert ops._grow_scratch(cache, cpu, 0) is second and ops._grow_scratch(cache, cpu, -1) is second
    assert synced == [cpu]
    # ... or, on an empty cache, 64 floats that are not kept
    for need in (0, -1):
        empty = {}
        dummy = ops._grow_scratch(empty, cpu, need)
        assert dummy.dtype == torch.float32 and dummy.numel() == 64 and not empty
    # int64 (ops.backward_workspace): rounded up to 8 bytes, the size compared in bytes
    wide = {}
    a = ops._grow_scratch(wide, cpu, 1001, torch.int64)
    assert a.dtype == torch.int64 and a.numel() == 126
    assert ops._grow_scratch(wide, cpu, 1008, torch.int64) is a
    assert ops._grow_scratch(wide, cpu, 1009, torch.int64).numel() == 127 and synced == [cpu, cpu]
