"""Flow-supervisor forward for the GMA variant (pytorch/core/gma_l2l.py:26-129).

Same two-phase schedule as core/l2l.py.  As in the reference, the second phase keeps calling ``update_block``
(gma_l2l.py:112); ``grad_update_block`` exists (and is part of the state_dict) but is not used by forward.
"""
from .gma_network import RAFTGMA
from .l2l import _FlowSupervisor
from .update import GMAUpdateBlock
from .._lib import on_tensor_device


class GMAL2L(_FlowSupervisor, RAFTGMA):
    def __init__(self, args):
        super().__init__(args)
        self.grad_update_block = GMAUpdateBlock(self.args, hidden_dim=self.hidden_dim)

    def _supervisor(self, n):
        """-> the supervisor phase stays on update_block (gma_l2l.py:112), and without a MotionBatch: as before, not a decision
        (core/l2l.py gives its supervisor phase one)."""
        return self.update_block, None

    def _uncropped_context(self, img):
        """-> (inp, attention) of an uncropped frame."""
        return self._context(img)[1:]

    @on_tensor_device
    def forward(self, image1, image2, ci1=None, ci2=None, ox=None, oy=None, iters=12, flow_init=None,
                upsample=True, test_mode=False, supervisor_grad=True, sup_grad_samples=None):
        return self._two_phase(image1, image2, ci1, ci2, ox, oy, iters, flow_init, test_mode, supervisor_grad, sup_grad_samples)
