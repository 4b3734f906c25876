"""QSpecEngine's slot bookkeeping on host tensors (no model, no GPU): the one stub the CPU tests share."""
import torch

from qspec_amd.spec_decode.engine import QSpecEngine
from qspec_amd.spec_decode.slot_sampling import SlotSampling


class HostEngine(QSpecEngine):
    def __init__(self, B=4, k=3, V=64):
        self.k, self.B, self.device = k, B, torch.device("cpu")
        self.blocks_per_seq, self.block_size, self.num_blocks = 16, 16, B * 16
        self.seq_lens = torch.zeros(B, dtype=torch.int32)
        self.gen_lens = torch.zeros(B, dtype=torch.int32)
        self._len_ub, self._gen_ub, self._bt_host = [0] * B, [0] * B, [None] * B
        self.sampling = SlotSampling(B, k, V, "cpu")
