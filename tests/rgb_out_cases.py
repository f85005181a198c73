"""Cases and expected values shared by tests/test_emu_rgb_out.py (CPU, through the emulator) and tests/test_gpu_rgb_out.py (device memory).

The expected picture comes from code that predates the colour-map entries: cityscapesLoader.decode_segmap of the label map sampled with the
frame loop's nearest rule, labels from the library's label entries.  Every comparison the two test files make is exact."""
import functools

import numpy as np

from ingest_u8_cases import ARGMAX_CASES, lowres_logits  # noqa: F401  (re-exported: the logits of the operator cases)
from tdnet_amd.dataloader import cityscapesLoader, nearest_index

# (n_src, n_dst) of the index tables
TABLE_PAIRS = [(33, 8), (65, 16), (33, 33), (33, 70), (9, 1), (1, 5), (769, 192), (1537, 384), (97, 200)]
# wider than one workgroup's strip (256 lanes x 4 pixels): GPU only.  (name, C, (h, w), (H, W), [(oh, ow), ...])
WIDE_CASES = [("wide", 19, (2, 300), (6, 2051), [(6, 2051), (3, 1030)]),
              ("native_769x1537", 19, (97, 193), (769, 1537), [(192, 384), (193, 385), (1024, 2048)])]


def old_index(n_src, n_dst):
    """The expression tdnet_amd/test.py's save() held inline before dataloader.nearest_index took it over."""
    return np.minimum((np.arange(n_dst) * (n_src / n_dst)).astype(np.int64), n_src - 1)


def out_sizes(H, W):
    """Per operator case: quarter, identity, an odd row of 51 bytes, an upscale, and three with ow < 4 (no aligned group fits)."""
    return [(H // 4, W // 4), (H, W), (7, 17), (H + 5, 2 * W + 1), (1, 1), (3, 2), (2, 3)]


def palette19():
    return np.array(cityscapesLoader.colors, np.uint8)


@functools.lru_cache(maxsize=None)
def palette40():
    p = np.random.default_rng(40).integers(0, 256, (40, 3), dtype=np.uint8)
    p.setflags(write=False)
    return p


def expected_picture(labels, oh, ow, palette=None):
    """decode_segmap(labels[ys][:, xs]).astype(uint8), ys / xs = dataloader.nearest_index (the frame loop's rule); palette: None = Cityscapes."""
    ld = cityscapesLoader(img_path="/nonexistent-frames", in_size=labels.shape)
    if palette is not None:
        ld.n_classes = len(palette)
        ld.label_colours = dict(zip(range(len(palette)), np.asarray(palette).tolist()))
    labels = np.asarray(labels)
    H, W = labels.shape
    return ld.decode_segmap(labels[nearest_index(H, oh)][:, nearest_index(W, ow)]).astype(np.uint8)


def logits40(h, w):
    """40 classes against the 19-colour palette: labels 19..39 come out grey."""
    x = np.random.default_rng(4000 + h * 10 + w).standard_normal((40, h, w)).astype(np.float32)
    return x
