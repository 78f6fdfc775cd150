"""What the CPU tests of the C ABI (tests/test_*_abi.py) share: the names a header declares, the strict-C99 check, the fake
context of the refusal tests, and the ctypes tables of all the binding modules for the "no name shared" assertions."""
import ctypes
import importlib
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

# every module of snark_verifier_amd with a ctypes table of device-library names, and the attribute that holds it
TABLES = {"_lib": "_SIGNATURES", "ipa_prover": "SIGNATURES", "ipa_batch": "SIGNATURES", "ipa_fold": "SIGNATURES",
          "ipa_create": "SIGNATURES", "poly": "SIGNATURES", "ipa_multiopen": "SIGNATURES", "ntt": "SIGNATURES",
          "poly_prod": "SIGNATURES", "quotient": "SIGNATURES", "lookup": "SIGNATURES"}


def declared(path, pattern=r"\b((?:snarkv|bn254|pallas)_[a-z0-9_]+)\s*\("):
    """the function names a header declares, sorted (comments set aside)"""
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(pattern, txt)))


def assert_strict_c99(header):
    """`header`: a path, or a file name under include/"""
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c",
                        os.path.join(INC, header)], capture_output=True, text=True)
    assert r.returncode == 0, os.path.basename(header) + ": " + r.stderr


def other_tables(module):
    """the names in the table of every binding module but the given one"""
    mine = module.__name__.rsplit(".", 1)[-1]
    assert mine in TABLES, mine
    names = set()
    for mod, attr in TABLES.items():
        if mod != mine:
            names |= set(getattr(importlib.import_module("snark_verifier_amd." + mod), attr))
    return names


class FakeKey(ctypes.Structure):
    """the head of the deciding key (csrc/ctx.hpp: device, k, points, first, count), enough for the argument checks
    that come before any device work; the calls of the tests never get past them"""
    _fields_ = [("device", ctypes.c_int), ("k", ctypes.c_uint32), ("d_points", ctypes.c_void_p), ("first", ctypes.c_size_t),
                ("count", ctypes.c_size_t), ("rest", ctypes.c_uint8 * 256)]


class FakeCtx(ctypes.Structure):
    """the head of the context (csrc/ctx.hpp: device first), enough for the checks that come before any device work"""
    _fields_ = [("device", ctypes.c_int), ("rest", ctypes.c_uint8 * 8192)]
