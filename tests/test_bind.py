"""CPU: the binder and the argument encoders the ctypes modules share (snark_verifier_amd._bind), against a stand-in library
object: no device, no library build."""
import ctypes

import pytest


class _Fn:
    restype = argtypes = None


class _FakeLib:
    def __init__(self, names):
        for n in names:
            setattr(self, n, _Fn())


SHAPES = {"thing_make": (ctypes.c_int, [ctypes.c_void_p]), "thing_size": (ctypes.c_size_t, [])}
FREE = {"bn254_thing_make": (ctypes.c_int, []), "pallas_thing_make": (ctypes.c_int, [ctypes.c_size_t])}


def test_a_missing_declared_name_is_an_attribute_error_that_names_it():
    from snark_verifier_amd import _bind

    whole = ["snarkv_thing_make", "snarkv_thing_size", "bn254_thing_make"]
    for missing in whole:
        with pytest.raises(AttributeError, match=missing):
            _bind.Api(_FakeLib([n for n in whole if n != missing]), "snarkv_", SHAPES, {"make_default": FREE})
    lib = _FakeLib(whole + ["snarkv_last_error"])
    api = _bind.Api(lib, "snarkv_", SHAPES, {"make_default": FREE})
    assert api.lib is lib and api.prefix == "snarkv_"
    assert api.thing_make is lib.snarkv_thing_make and api.make_default is lib.bn254_thing_make
    assert (api.thing_size.restype, api.thing_size.argtypes) == SHAPES["thing_size"]
    assert (api.make_default.restype, api.make_default.argtypes) == FREE["bn254_thing_make"]
    with pytest.raises(AttributeError, match="snarkv_thing_drop"):
        api.thing_drop


def test_binding_twice_returns_the_same_object(monkeypatch):
    from snark_verifier_amd import _bind

    libs = {False: _FakeLib(["snarkv_thing_make", "snarkv_thing_size", "bn254_thing_make"]),
            True: _FakeLib(["snarkv_pallas_thing_make", "snarkv_pallas_thing_size", "pallas_thing_make"])}
    monkeypatch.setattr(_bind, "_load_library", lambda pallas: libs[pallas])
    monkeypatch.setattr(_bind, "_BOUND", {})
    a = _bind.bind(SHAPES, {"make_default": FREE}, False)
    assert _bind.bind(SHAPES, {"make_default": FREE}, False) is a
    p = _bind.bind(SHAPES, {"make_default": FREE}, True)
    assert p is not a and p.prefix == "snarkv_pallas_" and p.make_default is libs[True].pallas_thing_make
    assert p.make_default.argtypes == [ctypes.c_size_t]


def test_check_raises_with_the_library_text():
    from snark_verifier_amd import SnarkvError, _bind

    lib = _FakeLib(["snarkv_thing_make", "snarkv_thing_size"])
    lib.snarkv_last_error = lambda: b"thing: no"
    api = _bind.Api(lib, "snarkv_", SHAPES)
    assert api.check(0) == 0 and api.check(3) == 3 and api.last_error() == "thing: no"
    with pytest.raises(SnarkvError, match="thing: no"):
        api.check(-2)


def test_the_encoders_of_addresses_indices_and_scalars():
    from snark_verifier_amd import _bind

    class _Tensor:
        def data_ptr(self):
            return 0x7000

    assert _bind.addr(None) is None
    a, t = _bind.addr(0x1230), _bind.addr(_Tensor())
    assert isinstance(a, ctypes.c_void_p) and a.value == 0x1230 and isinstance(t, ctypes.c_void_p) and t.value == 0x7000
    assert len(_bind.u32s([])) == 1 and list(_bind.u32s([7, 0xFFFFFFFF])) == [7, 0xFFFFFFFF]
    assert len(_bind.scalars([])) > 0
    assert _bind.scalars([1, b"\x02" + b"\x00" * 31]) == b"\x01" + b"\x00" * 31 + b"\x02" + b"\x00" * 31


def test_signatures_lists_a_table_under_both_prefixes():
    from snark_verifier_amd import _bind

    sig = _bind.signatures(SHAPES)
    assert sorted(sig) == ["snarkv_pallas_thing_make", "snarkv_pallas_thing_size", "snarkv_thing_make", "snarkv_thing_size"]
    assert sig["snarkv_thing_make"] is SHAPES["thing_make"] and sig["snarkv_pallas_thing_size"] is SHAPES["thing_size"]
