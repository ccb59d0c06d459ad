"""C-ABI library checks that need no GPU: it loads, exports every symbol the header
declares, the ctypes table matches the header, and argument validation fails cleanly
(no HIP call is made before validation)."""
import ctypes
import re

import pytest

from stereoanywhere_amd import _native as N


def header_functions():
    src = open(N.HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"^\s*(?:const\s+)?[\w\s\*]+?\b(sa_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = [a.strip() for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        out[m.group(1)] = len(args)
    return out


def test_library_exports_every_declared_symbol():
    lib = N.lib()
    decl = header_functions()
    assert len(decl) >= 20
    for name in decl:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"


def test_ctypes_table_matches_header():
    decl = header_functions()
    assert set(decl) == set(N.SIGNATURES), set(decl) ^ set(N.SIGNATURES)
    for name, nargs in decl.items():
        assert len(N.SIGNATURES[name][1]) == nargs, name


def test_pyramid_geometry():
    lib = N.lib()
    assert [lib.sa_pyramid_level_width(240, i) for i in range(4)] == [240, 120, 60, 30]
    assert [lib.sa_pyramid_level_offset(240, i) for i in range(4)] == [0, 240, 360, 420]
    assert lib.sa_pyramid_row_stride(240, 4) == 452
    # odd widths floor at every halving (avg_pool2d [1,2], corr.py:88-91)
    assert [lib.sa_pyramid_level_width(37, i) for i in range(4)] == [37, 18, 9, 4]
    assert lib.sa_pyramid_row_stride(37, 4) == 68


def test_argument_errors_are_reported():
    lib = N.lib()
    rc = lib.sa_corr_volume_pyramid(None, None, 1, 1, 1, 1, 1, 1.0, None, None, 0.9, 4, None, 4, None)
    assert rc == -1
    assert b"null pointer" in lib.sa_last_error()
    with pytest.raises(N.NativeError, match="num_levels"):
        N.call("sa_corr_lookup", 8, None, 32, 60, 7, 4, 8, 0, 1, 1, 1, 8, 100, None)


def test_timing_api_without_gpu():
    N.timing_enable(False)
    assert N.timing_read("corr_lookup") == (0.0, 0)


# ---------------------------------------------------------------- the bindings derived from the header
P, I, L, F, D = N.P, N.I, N.L, N.F, N.D


@pytest.mark.parametrize("name,want", [
    ("sa_corr_volume_pyramid", (I, [P, P, I, I, I, I, I, F, P, P, F, I, P, L, P])),
    ("sa_loss_terms_forward", (I, [I, P, P, P, P, I, I, I, D, I, D, D, P, P, P, P])),
    ("sa_last_error", (ctypes.c_char_p, [])),
    ("sa_lookup_set_mfma", (None, [I])),
    ("sa_conv3d_s2mf_weights_size", (L, [])),
    ("sa_timing_read", (I, [I, P, P])),
])
def test_signature_pins(name, want):
    """One literal signature per type form (int, long, float, double, pointers of every kind, the
    three return forms, an empty list): the parser's type rule against hand-read prototypes."""
    assert N.SIGNATURES[name] == want


def test_struct_pins():
    sizes = {"SaWinoProblem": 168, "SaGateEpilogue": 112, "SaResampleJob": 80, "SaFeatureGateJob": 80,
             "SaLossMap": 72}
    assert {n: ctypes.sizeof(s) for n, s in N.STRUCTS.items()} == sizes
    for n in sizes:
        assert getattr(N, n) is N.STRUCTS[n] and issubclass(N.STRUCTS[n], ctypes.Structure)
    assert N.SaWinoProblem._fields_ == [
        ("in_", P), ("in_bs", L), ("N", I), ("Cin", I), ("H", I), ("W", I), ("U", P), ("Cout", I), ("bias", P),
        ("relu", I), ("in_m", P), ("in_s", P), ("in_t", P), ("in_pstride", I), ("in_act", I), ("out", P),
        ("out_bs", L), ("stats_partial", P), ("pitch", I), ("skip", P), ("skip_bs", L), ("skip_s", P),
        ("skip_t", P), ("skip_act", I), ("out_act", I)]
    assert N.SaGateEpilogue._fields_ == [
        ("mode", I), ("ctx", P), ("ctx_bs", L), ("h", P), ("h_bs", L), ("z", P), ("z_bs", L), ("add", P),
        ("add_bs", L), ("out2", P), ("out2_bs", L), ("head_w", P), ("head_part", P), ("head_part_bs", L)]


def test_constants_and_kernel_names():
    assert N.ABI_VERSION == N.CONST["SA_ABI_VERSION"] == N.lib().sa_abi_version()
    assert N.CONST["SA_K_COUNT"] == 20 and N.CONST["SA_E_RUNTIME"] == -3 and N.CONST["SA_LOSS_DROP_NAN_BCE"] == 4
    lib = N.lib()
    assert N.KERNEL_IDS == {lib.sa_kernel_name(i).decode(): i for i in range(N.CONST["SA_K_COUNT"])}


SMALL = """
/* a comment with a prototype inside: int sa_not_this(unsigned x); */
#define SA_ABI_VERSION 3
#define SA_MASK 0x10   // trailing comment
enum { SA_STRUCT_TWO_WORDS = 0 };
enum { SA_A = 4, SA_B, SA_C, SA_M = -2, SA_Z };
typedef struct SaTwoWords {
  const float *in, *out;   /* a keyword field */
  int N, Cin;              // two declarators
  long in_bs;
  double w; float g;
} SaTwoWords;
int sa_abi_version(void);
const char *sa_name(int id);
void sa_set(int on, float x,
            double y, long n, const SaTwoWords *jobs, double *out);
"""


def test_parse_header_on_a_small_header():
    sig, structs, const = N.parse_header(SMALL)
    assert const == {"SA_ABI_VERSION": 3, "SA_MASK": 16, "SA_STRUCT_TWO_WORDS": 0, "SA_A": 4, "SA_B": 5, "SA_C": 6,
                     "SA_M": -2, "SA_Z": -1}
    assert list(structs) == ["SaTwoWords"]
    assert structs["SaTwoWords"]._fields_ == [("in_", P), ("out", P), ("N", I), ("Cin", I), ("in_bs", L), ("w", D),
                                              ("g", F)]
    assert sig == {"sa_abi_version": (I, []), "sa_name": (ctypes.c_char_p, [I]),
                   "sa_set": (None, [I, F, D, L, P, P])}


@pytest.mark.parametrize("text,named", [
    ("int sa_f(unsigned n);", "unsigned n"),
    ("int sa_f(unsigned int n);", "unsigned int n"),
    ("int sa_f(void (*cb)(int));", "sa_f"),
    ("float *sa_f(int n);", "sa_f"),
    ("int sa_f(int n[4]);", "n[4]"),
    ("int other(int n);", "other"),
    ("typedef struct { unsigned flags; } SaThing; enum { SA_STRUCT_THING = 0 };", "unsigned flags"),
    ("typedef struct { int (*cb)(int); } SaThing; enum { SA_STRUCT_THING = 0 };", "cb"),
    ("typedef struct { *a; } SaThing; enum { SA_STRUCT_THING = 0 };", "*a"),
    ("typedef struct { int a; } SaThing;", "SA_STRUCT_THING"),
    ("#define SA_X 1.5", "SA_X"),
    ("enum { SA_X = 1 << 2 };", "SA_X"),
])
def test_parse_header_refuses_what_it_cannot_type(text, named):
    with pytest.raises(N.NativeError) as e:
        N.parse_header(text)
    assert named in str(e.value)


def test_missing_header_is_a_native_error(monkeypatch, tmp_path):
    monkeypatch.setattr(N, "HEADER", str(tmp_path / "absent.h"))
    with pytest.raises(N.NativeError, match="absent.h"):
        N._read_header()
