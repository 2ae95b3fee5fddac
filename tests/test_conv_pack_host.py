"""CPU: csrc/conv3d_pack.h - the functions that give every element of the packed float32 convolution weights - compiled for the
HOST by g++ (tests/cpp/conv3d_pack_check.cpp) and compared with the float64 model of tests/conv_pack_model.py on the layers of
tests/conv_pack_cases.py.  tests/test_gpu_conv_pack.py asserts the same of the buffers the pack kernels write."""
import os
import subprocess

import numpy as np
import pytest

import conv_pack_cases as C
import conv_pack_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_case(path, c):
    with open(path, "wb") as f:
        np.array([c["cout"], c["cin"], c["cin_pad"], c["k"], c["transposed"], c["gamma"] is not None, c["b"] is not None], dtype=np.int32).tofile(f)
        np.array([c["eps"]], dtype=np.float32).tofile(f)
        for a in (c["w"], c["b"], c["gamma"], c["beta"], c["mean"], c["var"]):
            if a is not None:
                a.tofile(f)


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """{case: (wpack, bpack)} as the stand-alone program evaluates them: one build, one run over all cases."""
    d = tmp_path_factory.mktemp("conv_pack")
    exe = str(d / "conv3d_pack_check")
    subprocess.run(["g++", "-O2", "-o", exe, os.path.join(ROOT, "tests", "cpp", "conv3d_pack_check.cpp")], check=True)
    args = []
    for name in C.CASES:
        write_case(d / (name + ".in"), C.case(name))
        args += [str(d / (name + ".in")), str(d / (name + ".out"))]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for name in C.CASES:
        raw = np.fromfile(d / (name + ".out"), dtype=np.uint8)
        total = int(raw[:8].view(np.int64)[0])
        rest = raw[8:].view(np.float32)
        assert rest.size == total + M.round_up(C.case(name)["cout"], 16)
        out[name] = (rest[:total], rest[total:])
    return out


@pytest.mark.parametrize("name", list(C.CASES))
def test_header_packs_what_the_model_says(packed, name):
    M.check_packed(C.case(name), *packed[name])


def test_cases_reach_every_section_and_every_padding():
    seen = set()
    for name in C.CASES:
        c = C.case(name)
        _, _, pad, where = M.pack_model(c)
        seen |= set(where)
        for s, (at, n) in where.items():
            assert n > 0 and (s == "A" or pad[at:at + n].any() or c["cin"] == c["cin_pad"]), (name, s)
    assert seen == set("ABEFGHI")
    pads = lambda name, s: M.pack_model(C.case(name))[2][slice(*np.cumsum(M.pack_model(C.case(name))[3][s]))]
    assert pads("k7_c5_o16", "B").any() and pads("k7_c5_o16", "F").any() and pads("k7_c5_o16", "H").any()   # tap 343, taps 49-51, slot 147
    assert pads("k7_c7_o12", "A").any() and pads("k1_c32_o15", "A").any()                                   # couts >= cout
    assert pads("k3_c24_o64", "G").reshape(2, 4, -1)[:, 3].all()                                            # G's last 8-channel chunk


def test_a_wrong_element_is_told_from_a_right_one():
    c = C.case("k3_c5_o32")
    val, mag, pad, _ = M.pack_model(c)
    bval, _ = M.bias_model(c)
    good, gb = val.astype(np.float32), bval.astype(np.float32)
    M.check_packed(c, good, gb)
    i = int(np.argmax(mag))
    for bad in (np.nextafter(good[i], np.float32(np.inf), dtype=np.float32) + np.float32(64 * M.U) * np.abs(good[i]), np.float32("nan")):
        w = good.copy()
        w[i] = bad
        with pytest.raises(AssertionError):
            M.check_packed(c, w, gb)
    w = good.copy()
    w[int(np.argmax(pad))] = np.float32(1e-30)
    with pytest.raises(AssertionError):
        M.check_packed(c, w, gb)
    with pytest.raises(AssertionError):
        M.check_packed(c, good[:-256], gb)
