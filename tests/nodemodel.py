"""A numpy model of the touched-node exchange of ss_nodes.hip, shared by the protocol test (tests/test_dist_gloo.py, where
it stands in for the device) and the kernel tests (tests/test_nodes_exchange_gpu.py, where the device is compared with it)."""
import numpy as np
import torch


class NumpyNodes:
    """What ss_nodes_* gives dist.exchange_touched, on numpy arrays: a dense node-major buffer, touched flags, packing of
    the touched nodes' segments in node order.  The semantics of ss_nodes.hip (pack_offsets_kernel / pack_copy_kernel)."""

    def __init__(self, offsets, val, state=None):
        self._state = {} if state is None else state       # what the product keeps on the NodeSet: the learnt buffer size
        self.offsets = np.asarray(offsets, np.int64)
        self.n_nodes = self.offsets.size - 1
        self.val = val
        self.touched = np.zeros(self.n_nodes, np.int32)
        for j in range(self.n_nodes):
            self.touched[j] = int(val[self.offsets[j]:self.offsets[j + 1]].any())

    def flags_get(self, t, stream):
        t[:self.n_nodes] = torch.from_numpy(self.touched)

    def flags_set(self, t, stream):
        self.touched = t[:self.n_nodes].numpy().copy()

    def _segments(self):
        return [(int(self.offsets[j]), int(self.offsets[j + 1])) for j in range(self.n_nodes) if self.touched[j]]

    def pack(self, t, stream):
        seg = self._segments()
        n = sum(b - a for a, b in seg)
        if t is not None:
            assert t.numel() >= n
            o = 0
            for a, b in seg:
                t[o:o + b - a] = torch.from_numpy(self.val[a:b].view(np.int32))
                o += b - a
        return n

    def unpack(self, t, stream):
        o = 0
        for a, b in self._segments():
            self.val[a:b] = t[o:o + b - a].numpy().view(np.uint32)
            o += b - a

    # capped forms (ss_nodes_pack_capped_dev / ss_nodes_unpack_capped_dev): the first `cap` packed counts travel
    def pack_capped(self, t, cap, total_t, stream):
        o = 0
        for a, b in self._segments():
            m = max(0, min(b - a, cap - o))
            t[o:o + m] = torch.from_numpy(self.val[a:a + m].view(np.int32))
            o += b - a
        total_t[0] = o

    def unpack_capped(self, t, cap, stream):
        o = 0
        for a, b in self._segments():
            m = max(0, min(b - a, cap - o))
            self.val[a:a + m] = t[o:o + m].numpy().view(np.uint32)
            o += b - a

    @property
    def n_positions(self):
        return int(self.offsets[-1])

    @property
    def state(self):
        return self._state
