"""Host model of the PhysarumAgent population's decode (die_amd/csrc/die_physarum.hip `k_physarum_decode`, include/die_hip.h
`die_physarum_row`), written from its specification: (R, 6) float32 rows -> the decoded float32 values and the table rows —
what a stand-alone PhysarumAgent of those constructor arguments hands the kernels, and the constants die_fill_fwd_args derives
from them.  numpy float32 / Python float64 arithmetic, one rounding per operation."""
import math
import struct

import numpy as np

f32 = np.float32
NAMES = ('scale', 'deposit', 'sense_offset', 'turn_angle', 'sense_angle', 'turn_tolerance')
ROW_FIELDS = ('scale', 'deposit', 'sense_offset', 'c_turn', 'c_sense', 'turn_radians', 'sense_radians', 'turn_tolerance', 'x_turn', 'atol')


def decode_values(rows, lo=None, hi=None) -> np.ndarray:
    """Natural rows (lo is None): the rows.  Unit rows: lo + (hi − lo)·clamp(u, 0, 1), the product and the sum each rounded
    to float32; a NaN coordinate reads as 0."""
    u = np.asarray(rows, dtype=f32)
    if lo is None:
        return u.copy()
    lo, hi = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)
    c = np.fmin(np.fmax(u, f32(0)), f32(1))
    span = (hi - lo).astype(f32)
    t = (span * c).astype(f32)
    return (lo + t).astype(f32)


def _bits(x: float) -> int:
    return struct.unpack('<Q', struct.pack('<d', x))[0]


def _double(b: int) -> float:
    return struct.unpack('<d', struct.pack('<Q', b))[0]


def isclose_bound(atol: float, rtol: float) -> float:
    """Largest x >= 0 with x <= atol + rtol·x (np.isclose(0, x, rtol, atol)), by bisection over the doubles' bit patterns."""
    ok = lambda x: x <= atol + rtol * x
    if not ok(0.0):
        return -1.0
    if not rtol < 1.0:
        return math.inf
    top = 2.0 * atol / (1.0 - rtol) + 1e-300
    if ok(top):
        return math.inf
    lo, hi = 0, _bits(top)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if ok(_double(mid)):
            lo = mid
        else:
            hi = mid
    return _double(lo)


def table_row(v) -> dict:
    """One table row from six decoded float32 values."""
    v = [float(f32(q)) for q in v]
    turn, sense, rtol = math.radians(v[3]), math.radians(v[4]), v[5]
    atol = turn * rtol
    x_turn = isclose_bound(atol, 1e-2)
    c = lambda x: f32(2.0) if x < 0.0 else (f32(-2.0) if x >= math.pi else f32(math.cos(x)))
    return dict(scale=f32(v[0]), deposit=f32(v[1]), sense_offset=f32(v[2]), c_turn=c(x_turn), c_sense=c(sense), turn_radians=turn,
                sense_radians=sense, turn_tolerance=rtol, x_turn=x_turn, atol=atol)


def decode(rows, lo=None, hi=None):
    """(values (R, 6) float32, [table_row of every replica])."""
    values = decode_values(rows, lo, hi)
    return values, [table_row(v) for v in values]
