"""Shared by the tests of the persistent workspaces (test_gpu_persist.py,
test_gpu_workspace_lifetime.py, test_gpu_harness.py): the flow fields of
their call sequences and the pressure that empties the workspace cache."""
import gc

import numpy as np


def np_fields(B, H, W):
    """Decoder-style flows as numpy: a smooth +-2 px field with a per-sample
    phase, a border-piling shift (a strip of sources clamped onto the edge
    column: many pixels per cell), and a field contracting towards the centre
    (whole regions share a cell: overflow entries and dirty tiles)."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    ph = np.arange(B, dtype=np.float32).reshape(B, 1, 1) * 0.7
    u = np.sin(2 * np.pi * 2 * xx / W + ph) + np.cos(2 * np.pi * 3 * yy / H - ph)
    v = np.cos(2 * np.pi * 2 * xx / W - ph) - np.sin(2 * np.pi * 3 * yy / H + ph)
    smooth = np.stack([u, v], 1).astype(np.float32)
    pile = smooth.copy()
    pile[:, 0] += W / 8.0
    contract = np.stack([0.9 * ((W - 1) / 2.0 - xx), 0.9 * ((H - 1) / 2.0 - yy)])[None].repeat(B, 0)
    return {"smooth": smooth, "pile": pile, "contract": contract.astype(np.float32)}


def cache_pressure(dev, key=None):
    """Everything that takes a workspace out of ops' cache: more other shapes
    than the cache keeps (least recently used out), the failed-call drop of
    ``key`` = (device index, op, shape), a clear, and a garbage collection."""
    from unsamflow_amd import ops

    for i in range(ops.PERSIST_MAX_ENTRIES + 5):
        ops.persistent_workspace(dev, "test_op", (i,), 64)
    if key is not None:
        ops._drop_workspace(dev, key[1], key[2])
    ops.clear_persistent_workspaces()
    gc.collect()
