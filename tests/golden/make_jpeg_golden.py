"""Golden fixture of the JPEG recompression stage of the device augmentation chain: ``augment_jpeg.npz``.

Pillow's results for the grid of ``tests/jpeg_helpers.py`` (``cases()``), produced through the REFERENCE's own
``VideoFacesDataset._RandomJPEGCompression`` (``src/dataset.py:83-105``, imported from a checkout of the reference
under a stub ``torchvision.transforms``; development machine only) with ``random.random`` patched to 0.0 (always
apply) and ``random.randint`` to the case's quality.  Small cases store the source and the whole result;
224 x 224 results store a CRC-32 and three rows, and their sources are regenerated from their seeds.  Also
recorded: Pillow's version and the version of the JPEG library it was built with.

    python tests/golden/make_jpeg_golden.py /path/to/reference
"""
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import PIL  # noqa: E402
from PIL import Image, features  # noqa: E402

import jpeg_helpers as jh  # noqa: E402


def main():
    ref = sys.argv[1]
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.path.insert(0, os.path.join(ref, "src"))
    from dataset import VideoFacesDataset  # noqa: E402

    stage = VideoFacesDataset._RandomJPEGCompression(p=0.5, quality_min=35, quality_max=95)
    out = {"pillow_version": np.array(PIL.__version__), "jpeg_version": np.array(str(features.version("jpg"))),
           "libjpeg_turbo": np.array([int(bool(features.check_feature("libjpeg_turbo")))], np.int64)}
    random.random = lambda: 0.0
    for name, shape, content, q in jh.cases():
        a = jh.source(shape, content)
        random.randint = lambda lo, hi, q=q: q
        want = np.array(stage(Image.fromarray(a).convert("RGB")))
        assert want.shape == (*shape, 3) and want.dtype == np.uint8
        if shape == (224, 224):
            out[f"crc/{name}"] = jh.digest(want)
            out[f"rows/{name}"] = want[list(jh.GOLDEN_ROWS)]
        else:
            out[f"src/{jh.src_key(shape, content)}"] = a
            out[f"out/{name}"] = want
    path = os.path.join(HERE, "augment_jpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__, "jpeg", features.version("jpg"))


if __name__ == "__main__":
    main()
