"""felics_get_decode_stats: the entry point is exported and listed, refuses NULL arguments, and the Python mirror of
felics_decode_stats has the C struct's layout (no GPU needed: the refusals come before anything touches a device)."""
import ctypes as C
import os
import re

E_INVALID_ARGUMENT = -11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_fields():
    """the members of felics_decode_stats as include/felics.h declares them (all uint64_t)"""
    text = open(os.path.join(ROOT, "include", "felics.h")).read()
    body = re.search(r"typedef struct felics_decode_stats \{(.*?)\} felics_decode_stats;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("uint64_t "), decl
        names += [n.strip() for n in decl[len("uint64_t "):].split(",")]
    return names


def test_decode_stats_abi_surface():
    from felics_amd import api

    L = api.lib()
    for name in ("felics_get_decode_stats", "felics_decode_lanes_min_streams"):
        assert hasattr(L, name), name
        assert name in api.EXPORTS
    st = api._CDecodeStats(*([7] * 8))
    assert L.felics_get_decode_stats(None, C.byref(st), C.sizeof(st)) == E_INVALID_ARGUMENT
    assert [getattr(st, n) for n, _ in api._CDecodeStats._fields_] == [7] * 8  # nothing written
    fake = C.c_void_p(16)  # never dereferenced: `out` is checked first
    assert L.felics_get_decode_stats(fake, None, C.sizeof(st)) == E_INVALID_ARGUMENT
    assert L.felics_get_decode_stats(None, None, 0) == E_INVALID_ARGUMENT
    assert callable(getattr(api.Encoder, "decode_stats", None))
    assert api.decode16_lanes_min_streams(0) > 64 and api.decode16_lanes_min_streams(1) > 64


def test_decode_stats_struct_layout():
    from felics_amd import api

    names = _c_fields()
    assert names == ["streams", "wave8", "lanes8", "wave16", "lanes16", "host", "undecoded", "lanes16_table_bytes"]
    assert [n for n, _ in api._CDecodeStats._fields_] == names
    assert all(t is C.c_uint64 for _, t in api._CDecodeStats._fields_)
    assert C.sizeof(api._CDecodeStats) == 8 * len(names) == 64
