"""Layers for the packed-weight tests (tests/test_conv_pack_host.py, tests/test_gpu_conv_pack.py): the smallest ones that reach
every section of the buffer se_conv3d_pack_f32 writes (csrc/conv3d_pack.h) and every kind of zero padding in it.

A case is (cout, cin, cin_pad, k, transposed, BatchNorm?, bias?)."""
import functools

import numpy as np

BN, NO_BN, BIAS, NO_BIAS = True, False, True, False

CASES = {
    "k3_c5_o32":   (32, 5, 16, 3, 0, BN, BIAS),           # A C E G I; channels >= cin zero
    "k3_c24_o64":  (64, 24, 32, 3, 0, NO_BN, NO_BIAS),    # two cout blocks; G's last 8-channel chunk all zero
    "k3_c16_o48":  (48, 16, 16, 3, 0, BN, BIAS),          # A only; odd nts
    "k1_c32_o15":  (15, 32, 32, 1, 0, NO_BN, BIAS),       # cout padding; bpack[15] == 0
    "k7_c5_o16":   (16, 5, 16, 7, 0, BN, BIAS),           # A B D F H; 3- and 4-channel chunk tails; tap padding
    "k7_c7_o12":   (12, 7, 16, 7, 0, BN, NO_BIAS),        # cout < 16
    "k7_c16_o32":  (32, 16, 16, 7, 0, BN, BIAS),          # A B only; nts 2
    "t2_c32_o16":  (16, 32, 32, 2, 1, BN, BIAS),          # transposed
    "t2_c16_o48":  (48, 16, 16, 2, 1, BN, BIAS),          # transposed index order
}
EPS = 1e-5


@functools.lru_cache(maxsize=None)
def case(name):
    """Seeded float32 inputs of a case: w [cout][cin][k^3] (transposed: [cin][cout][8]); b, gamma, beta, mean, var [cout] or None.
    gamma and var are positive and away from 0."""
    cout, cin, cin_pad, k, transposed, bn, bias = CASES[name]
    rng = np.random.default_rng(1000 + list(CASES).index(name))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    shape = (cin, cout, 8) if transposed else (cout, cin, k ** 3)
    c = dict(name=name, cout=cout, cin=cin, cin_pad=cin_pad, k=k, transposed=transposed, eps=EPS,
             w=f(rng.standard_normal(shape)), b=f(rng.standard_normal(cout)) if bias else None,
             gamma=None, beta=None, mean=None, var=None)
    if bn:
        c.update(gamma=f(rng.uniform(0.5, 1.5, cout)), beta=f(rng.standard_normal(cout)), mean=f(rng.standard_normal(cout)),
                 var=f(rng.uniform(0.5, 2.0, cout)))
    return c
