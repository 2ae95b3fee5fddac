"""GPU: the buffers se_conv3d_pack_f32 writes (csrc/conv3d_pack.hip), element by element, against the float64 model of
tests/conv_pack_model.py on the layers of tests/conv_pack_cases.py.  wpack and bpack are filled with NaN before the call;
tests/test_conv_pack_host.py asserts the same of the header's functions on the CPU."""
import numpy as np
import pytest
import torch

import conv_pack_cases as C
import conv_pack_model as M
from sceneego_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(C.CASES))
def test_pack_writes_what_the_model_says(name):
    c = C.case(name)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    total = _lib.conv3d_packed_elems(c["cout"], c["cin_pad"], c["k"], c["transposed"])
    assert total == sum(M.section_sizes(c["cout"], c["cin_pad"], c["k"], c["transposed"]).values())
    wpack = torch.full((total,), float("nan"), device=DEV)
    bpack = torch.full((M.round_up(c["cout"], 16),), float("nan"), device=DEV)
    _lib.conv3d_pack(dev(c["w"]), dev(c["b"]), dev(c["gamma"]), dev(c["beta"]), dev(c["mean"]), dev(c["var"]), c["eps"], wpack, bpack,
                     c["cout"], c["cin"], c["cin_pad"], c["k"], c["transposed"])
    torch.cuda.synchronize()
    M.check_packed(c, wpack.cpu().numpy(), bpack.cpu().numpy())
