"""The quotient polynomial on the extended coset (include/snarkv_quotient.h), over a BN254 `Context` or a pallas
`PallasContext`: coefficient columns to their values on the coset (`extend_dev`), a straight-line gate program run at every
row (`eval_dev`), the division by the vanishing polynomial (`div_vanishing_dev`), and the three with the inverse transform in
one call (`quotient_dev`); and the same quotient one coset of the small domain at a time, over a work buffer 2^e times smaller
(`cosets_dev`, with its last step `cosets_join_dev`: include/snarkv_quotient_cosets.h).  Every call enqueues on the context's stream and returns; the caller synchronises before it reads a
result.

Columns are device addresses (ints, or anything with `data_ptr()`); shifts and constants are ints or 32-byte strings.  A
program is a `Program`, or a pair (packed instructions, list of constants).

The ctypes tables are this module's own, as `poly_prod`'s and `ntt`'s are: one table per header.
"""
import ctypes
import struct

from ._bind import addr as _addr, bind, fe as _fe, is_pallas, signatures

_vp, _cp, _sz, _int, _u32 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32

REGS = 16  # SNARKV_QUOT_REGS
MAX_INSTR, MAX_CONSTS, MAX_COLS, MAX_E = 4096, 1024, 1 << 20, 8  # SNARKV_QUOT_MAX_*
ADD, SUB, MUL, FMA = 0, 1, 2, 3  # SNARKV_QUOT_ADD ...
INSTR_BYTES = 16  # sizeof(snarkv_quot_instr)

# name without the library prefix -> (restype, argtypes)
_SHAPES = {
    "poly_extend_dev": (_int, [_vp, _vp, _u32, _u32, _sz, _cp, _vp]),
    "quotient_eval_dev": (_int, [_vp, _vp, _u32, _u32, _sz, _cp, _sz, _cp, _sz, _vp]),
    "poly_div_vanishing_dev": (_int, [_vp, _vp, _u32, _u32, _cp, _vp]),
    "quotient_dev": (_int, [_vp, _vp, _u32, _u32, _sz, _cp, _sz, _cp, _sz, _cp, _cp, _vp, _vp]),
}
# every function include/snarkv_quotient.h declares
SIGNATURES = signatures(_SHAPES)


# ... and include/snarkv_quotient_cosets.h
_COSETS_SHAPES = {
    "quotient_cosets_dev": _SHAPES["quotient_dev"],
    "poly_cosets_join_dev": (_int, [_vp, _vp, _u32, _u32, _cp, _vp]),
}
COSETS_SIGNATURES = signatures(_COSETS_SHAPES)


def api(pallas):
    """the functions of one library (`pallas`: the pasta build)"""
    return bind(_SHAPES, None, pallas)


def cosets_api(pallas):
    """the functions of include/snarkv_quotient_cosets.h in one library"""
    return bind(_COSETS_SHAPES, None, pallas)


def REG(i):
    """SNARKV_QUOT_REG: register i"""
    return i & 0xFFFFFFFF


def CONST(i):
    """SNARKV_QUOT_CONST: constant i"""
    return (1 << 30) | (i & 0xFFFFFFFF)


def COL(col, rot=0):
    """SNARKV_QUOT_COL: column `col` at the row `rot` domain steps away, -512 <= rot <= 511"""
    return (2 << 30) | ((rot & 0x3FF) << 20) | (col & 0xFFFFF)


def pack_instr(op, dst, a, b, c=0, zero=0):
    """one snarkv_quot_instr"""
    return struct.pack("<BBHIII", op, dst, zero, a, b, c)


class Program:
    """A gate program under construction: instructions are appended as they are named, constants are kept once each."""

    def __init__(self):
        self.instrs = []  # (op, dst, a, b, c)
        self.consts = []  # ints
        self._const_at = {}

    def const(self, value):
        """the operand word of the constant `value` (an int), added on its first use"""
        value = int(value)
        if value not in self._const_at:
            self._const_at[value] = len(self.consts)
            self.consts.append(value)
        return CONST(self._const_at[value])

    def _emit(self, op, dst, a, b, c=0):
        self.instrs.append((op, dst, a, b, c))
        return REG(dst)

    def add(self, dst, a, b):
        return self._emit(ADD, dst, a, b)

    def sub(self, dst, a, b):
        return self._emit(SUB, dst, a, b)

    def mul(self, dst, a, b):
        return self._emit(MUL, dst, a, b)

    def fma(self, dst, a, b, c):
        return self._emit(FMA, dst, a, b, c)

    def __len__(self):
        return len(self.instrs)

    def packed(self):
        """the instructions as the bytes of a snarkv_quot_instr array"""
        return b"".join(pack_instr(*i) for i in self.instrs)


def _program(prog):
    """-> (instruction bytes, n_instr, constant bytes, n_consts)"""
    code, consts = (prog.packed(), prog.consts) if isinstance(prog, Program) else prog
    assert len(code) % INSTR_BYTES == 0
    return code or b"\x00", len(code) // INSTR_BYTES, b"".join(_fe(v) for v in consts) or b"\x00", len(consts)


def extend_dev(ctx, d_coeffs, k, e, count, shift, d_out):
    """out[p][i] = f_p(shift * W^i) over the 2^(k+e) domain, for `count` polynomials of 2^k coefficients"""
    a = api(is_pallas(ctx))
    a.check(a.poly_extend_dev(ctx._h, _addr(d_coeffs), k, e, count, _fe(shift), _addr(d_out)))


def eval_dev(ctx, d_cols, k, e, n_cols, prog, d_out):
    """out[i] = the program's last destination register at row i of the `n_cols` columns of 2^(k+e) values"""
    a = api(is_pallas(ctx))
    code, n_instr, consts, n_consts = _program(prog)
    a.check(a.quotient_eval_dev(ctx._h, _addr(d_cols), k, e, n_cols, code, n_instr, consts, n_consts, _addr(d_out)))


def div_vanishing_dev(ctx, d_in, k, e, shift, d_out):
    """out[i] = in[i] / ((shift * W^i)^(2^k) - 1); out may be in"""
    a = api(is_pallas(ctx))
    a.check(a.poly_div_vanishing_dev(ctx._h, _addr(d_in), k, e, _fe(shift), _addr(d_out)))


def quotient_dev(ctx, d_coeffs, k, e, n_cols, prog, shift, shift_inv, d_work, d_h):
    """h = the 2^(k+e) coefficients of (the program over the extended columns) / (X^(2^k) - 1); d_work holds
    n_cols * 2^(k+e) elements"""
    a = api(is_pallas(ctx))
    code, n_instr, consts, n_consts = _program(prog)
    a.check(a.quotient_dev(ctx._h, _addr(d_coeffs), k, e, n_cols, code, n_instr, consts, n_consts, _fe(shift), _fe(shift_inv),
                           _addr(d_work), _addr(d_h)))


def cosets_dev(ctx, d_coeffs, k, e, n_cols, prog, shift, shift_inv, d_work, d_h):
    """`quotient_dev`'s h, byte for byte, one coset of the 2^k domain at a time; d_work holds n_cols * 2^k elements"""
    a = cosets_api(is_pallas(ctx))
    code, n_instr, consts, n_consts = _program(prog)
    a.check(a.quotient_cosets_dev(ctx._h, _addr(d_coeffs), k, e, n_cols, code, n_instr, consts, n_consts, _fe(shift), _fe(shift_inv),
                                  _addr(d_work), _addr(d_h)))


def cosets_join_dev(ctx, d_vals, k, e, shift_inv, d_out):
    """2^e rows of 2^k values, row j the values on the coset (s W^j) H -> the 2^(k+e) coefficients of the polynomial; out may be
    the input"""
    a = cosets_api(is_pallas(ctx))
    a.check(a.poly_cosets_join_dev(ctx._h, _addr(d_vals), k, e, _fe(shift_inv), _addr(d_out)))
