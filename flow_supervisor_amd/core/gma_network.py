"""RAFT-GMA forward (pytorch/core/gma_network.py:26-129) on the HIP hot path (benchmark config 5)."""
from .corr import CorrBlock
from .extractor import BasicEncoder
from .gma import Attention
from .raft import _Shell, normalise
from .update import GMAUpdateBlock
from .._lib import on_tensor_device


class RAFTGMA(_Shell):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.hidden_dim = hdim = 128
        self.context_dim = cdim = 128
        args.corr_levels = 4
        args.corr_radius = 4
        if "dropout" not in self.args:
            self.args.dropout = 0
        if "mixed_precision" not in self.args:
            self.args.mixed_precision = False
        from .utils.utils import warn_mixed_precision
        warn_mixed_precision(self.args)
        self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=args.dropout)
        self.cnet = BasicEncoder(output_dim=hdim + cdim, norm_fn="batch", dropout=args.dropout)
        self.cnet.out_channels_last = True   # the context features reach the update block channels_last (extractor._Encoder.forward)
        self.update_block = GMAUpdateBlock(self.args, hidden_dim=hdim)
        self.att = Attention(args=self.args, dim=cdim, heads=self.args.num_heads, max_pos_size=160, dim_head=cdim)

    def _corr_block(self, fmap1, fmap2):
        """Always the all-pairs block: the GMA networks do not read args.alternate_corr (gma_network.py:90)."""
        return CorrBlock(fmap1, fmap2, radius=self.args.corr_radius)

    def _context(self, img):
        """-> (net, inp) channels-last and the attention map of inp (consumed by update_block.forward_cl only)."""
        net, inp, _ = super()._context(img)
        return net, inp, self.att.forward_cl(inp, records=True)

    @on_tensor_device
    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True, test_mode=False):
        return self._single_phase(normalise(image1), normalise(image2), iters, flow_init, test_mode)
