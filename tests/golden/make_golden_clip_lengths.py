#!/usr/bin/env python
"""G8: the whole-tile results of the four temporal-attention entry points (fmc_temporal_attn_fwd / _bwd in bf16 and fp32 storage,
fmc_temporal_attn_fp8_fwd / _bwd) at F = 16 and F = 32 on the fixed inputs of `tests/clip_lengths_common.py`, as raw bits.  Recorded on an
MI355X with the library built from the commit BEFORE the kernels learnt partial frame tiles (`FMC_HIP_LIB` selects the build; the Python
layer of the entry points did not change), so that tests/test_gpu_clip_lengths.py::test_full_tiles_bit_identical can assert that the
16- and 32-frame paths did not move by one bit.  (The forward arrays of the committed files are from the library that
normalises on the PV accumulator, profiles/attn_forward_bounds.md; the backward arrays from the earlier one.)  Needs the GPU; writes data only:

    FMC_HIP_LIB=/path/to/the/earlier/libfmc_hip.so python tests/golden/make_golden_clip_lengths.py [output directory]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np


def main():
    from synfmc_amd import _lib, hip_ops as K
    from tests import clip_lengths_common as CL
    dst = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(dst, exist_ok=True)
    print(f"library: {_lib.LIB_PATH}", flush=True)
    for Fr in (16, 32):
        out = CL.full_tile_outputs(K, Fr)
        path = os.path.join(dst, f"g8_temporal_attn_full_tiles_f{Fr}.npz")
        np.savez_compressed(path, shape=np.array([CL.GOLD_B, Fr, CL.GOLD_P, CL.GOLD_H, CL.GOLD_D]), **out)
        print(f"F = {Fr}: {', '.join(f'{k} {v.shape}' for k, v in out.items())} -> {path} ({os.path.getsize(path)} bytes)", flush=True)


if __name__ == "__main__":
    main()
