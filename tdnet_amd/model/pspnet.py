"""`from model import pspnet; pspnet.pspnet(nclass=19, model_path=...)` -- Testing/test.py:34-38 (`--model psp101`).

Mirror of Testing/model/pspnet/pspnet.py:31-115: the stateless single-frame PSPNet the reference uses as its comparison
model (ResNet-101 dilated multi-grid backbone + PSPHead = full pyramid pooling, conv3x3 4096->512, classifier).  It reuses
the TDNet kernels (Bottleneck convs, pyramid pooling, head, upsample); `pos_id` is accepted and ignored like in the
reference (pspnet.py:73).  Every backbone the constructor accepts runs (pspnet.py:50-67): ResNet-18 / 34 with the 7x7 stem and
PSPHead(512) (pyramid 512 -> 4 x 128, conv3x3 1024 -> 128), ResNet-50 / 101 with the deep stem and PSPHead(2048); `dilated` /
`multi_grid` as for the TDNet classes."""
import torch

from ._base import _TDNetBase
from .. import arch


class pspnet(_TDNetBase):
    _model_id = 1
    _spec_name = "psp"

    def __init__(self, nclass=21, norm_layer=None, backbone="resnet101", dilated=True, aux=True, multi_grid=True,
                 model_path=None, synthetic_seed=None, kernel_opts=None):
        if backbone not in ("resnet18", "resnet34", "resnet50", "resnet101"):
            raise RuntimeError("unknown backbone: {}".format(backbone))             # pspnet.py:65-66
        torch.nn.Module.__init__(self)
        self.psp_path = model_path
        self.path_num = 1
        self.nclass = nclass
        self.backbone = backbone
        self.dilated, self.multi_grid = bool(dilated), bool(multi_grid)
        self.synthetic_seed = synthetic_seed
        self.kernel_opts = dict(kernel_opts or {})
        self._pending_shape = None
        self.spec = arch.model_spec("psp", nclass, backbone, self.dilated, self.multi_grid)
        self._state = None
        self._engine = None
        self._engine_key = None
        self._init_batch_state()
        self.pretrained_mp_load()

    def forward(self, x, pos_id=None):
        return super().forward(x[-1:], 0)                                          # pspnet.py:74: x = x[-1:]

    def forward_labels(self, x, pos_id=None):
        return super().forward_labels(x[-1:], 0)

    def forward_u8(self, x, pos_id=None, **kw):
        return super().forward_u8(x[-1:], 0, **kw)

    def forward_labels_u8(self, x, pos_id=None, **kw):
        return super().forward_labels_u8(x[-1:], 0, **kw)

    def forward_rgb(self, x, pos_id=None, out_size=None, palette=None):
        return super().forward_rgb(x[-1:], 0, out_size, palette)

    def forward_rgb_u8(self, x, pos_id=None, in_size=None, out_size=None, **kw):
        return super().forward_rgb_u8(x[-1:], 0, in_size, out_size, **kw)

    def forward_score(self, x, gt_u8, pos_id=None, **kw):
        return super().forward_score(x[-1:], gt_u8[-1:], 0, **kw)

    def forward_score_u8(self, x, gt_u8, pos_id=None, in_size=None, **kw):
        return super().forward_score_u8(x[-1:], gt_u8[-1:], 0, in_size, **kw)

    def forward_labels_conf(self, x, pos_id=None):
        return super().forward_labels_conf(x[-1:], 0)

    def forward_labels_conf_u8(self, x, pos_id=None, in_size=None, **kw):
        return super().forward_labels_conf_u8(x[-1:], 0, in_size, **kw)

    def forward_nv12(self, x, pos_id=None, src_size=None, **kw):
        return super().forward_nv12(x[-1:], 0, src_size, **kw)

    def forward_labels_nv12(self, x, pos_id=None, src_size=None, **kw):
        return super().forward_labels_nv12(x[-1:], 0, src_size, **kw)

    def forward_rgb_nv12(self, x, pos_id=None, src_size=None, in_size=None, out_size=None, **kw):
        return super().forward_rgb_nv12(x[-1:], 0, src_size, in_size, out_size, **kw)

    def forward_score_nv12(self, x, gt_u8, pos_id=None, src_size=None, **kw):
        return super().forward_score_nv12(x[-1:], gt_u8[-1:], 0, src_size, **kw)

    def forward_labels_conf_nv12(self, x, pos_id=None, src_size=None, **kw):
        return super().forward_labels_conf_nv12(x[-1:], 0, src_size, **kw)
