"""Writes tests/golden/libm_cr.npz: the correctly rounded pow, sin and cos of the operands of
tests/prim_model.py (pow_operands, trig_operands; N_FIXTURE of each), computed with mpmath at 200 bits and
rounded once to float64, to nearest even.

To stay no larger than the other fixtures the file does not hold the 20,000 operands and results as float64
(0.8 MB of incompressible mantissas).  It holds
  * per function the low 16 bits of every result's ordinal (prim_model.ordinal: float64 values numbered in
    order), as uint16: a value within 2^15 representable values of the correctly rounded one has its distance
    from it in those bits, and the tests that read them first bound the value by the host libm in full;
  * the operands' CRC-32, so that a reader knows it formed the same operands (they are a pure function of
    their index).

Run from the repository root:  python tests/golden/make_libm_fixtures.py   (needs mpmath >= 1.3)
"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import prim_model as pm  # noqa: E402

PREC = 200


def correctly_rounded(fn, *operands):
    """fn ('pow' | 'sin' | 'cos') of float64 operand arrays -> float64, rounded once from PREC bits."""
    import mpmath
    mpmath.mp.prec = PREC
    f = {"pow": mpmath.power, "sin": mpmath.sin, "cos": mpmath.cos}[fn]
    out = np.empty(len(operands[0]), np.float64)
    for i, args in enumerate(zip(*operands)):
        r = f(*[mpmath.mpf(float(a)) for a in args])
        # one rounding of the 200-bit value to 53 bits, to nearest even (exact for a normal result)
        out[i] = mpmath.libmp.to_float(r._mpf_, rnd=mpmath.libmp.round_nearest)
    assert np.all((np.abs(out) >= 2.0 ** -1022) | (out == 0.0)), "a subnormal result would be rounded twice"
    return out


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a, np.float64).tobytes())


def low16(x):
    return (pm.ordinal(x) & 0xFFFF).astype(np.uint16)


def main():
    n = pm.N_FIXTURE
    c, y = pm.pow_operands(n)
    x = pm.trig_operands(n)
    res = {"pow": correctly_rounded("pow", c, y), "sin": correctly_rounded("sin", x), "cos": correctly_rounded("cos", x)}
    np.savez_compressed(os.path.join(HERE, "libm_cr.npz"), n=np.int64(n), prec=np.int64(PREC),
                        operands_crc=np.array([crc(c), crc(y), crc(x)], np.int64),
                        **{k + "_low16": low16(v) for k, v in res.items()})


if __name__ == "__main__":
    main()
