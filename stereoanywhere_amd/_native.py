"""ctypes binding of libsa_hip.so, derived from the C ABI's one declaration.

include/stereoanywhere_hip.h is the only place an entry point, a struct or a constant is declared:
the .hip sources include it (the compiler checks each definition against it) and this module parses
it at import into SIGNATURES, the Sa* ctypes structures and CONST.  A new entry point needs the
header, its .hip definition and its ops wrapper, and nothing here.

The library is built in-tree (``make`` or ``stereoanywhere_amd._native.build()``) so the
.so travels with the repo snapshot to the GPU box.  There is no fallback: if the
library is missing every op raises, loudly.
"""
from __future__ import annotations

import ctypes
import keyword
import os
import re
import shlex
import subprocess
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("SA_HIP_LIB") or os.path.join(_HERE, "lib", "libsa_hip.so")  # override: A/B runs
HEADER = os.path.join(ROOT, "include", "stereoanywhere_hip.h")

P = ctypes.c_void_p
I = ctypes.c_int
L = ctypes.c_long
F = ctypes.c_float
D = ctypes.c_double


class NativeError(RuntimeError):
    pass


_H = "include/stereoanywhere_hip.h"
_SCALAR = {"int": I, "long": L, "float": F, "double": D}
# [const] base-type [stars] [name]: one parameter, or the head of a struct field line
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*)*)(\w*)")
_DECLARATOR = re.compile(r"((?:\*\s*)*)(\w+)")


def _ctype(base: str, stars: str, decl: str):
    """The type rule: any pointer is a void pointer, the four scalars map to their ctypes, and
    anything else (unsigned, a struct by value, ...) is refused."""
    if stars:
        return P
    if base not in _SCALAR:
        raise NativeError(f"{_H}: cannot type `{decl}`")
    return _SCALAR[base]


def _struct_id(name: str) -> str:
    """SaFeatureGateJob -> SA_STRUCT_FEATURE_GATE_JOB (the id sa_struct_size takes)."""
    return "SA_STRUCT_" + re.sub(r"(?<!^)(?=[A-Z])", "_", name[2:]).upper()


def parse_header(text: str):
    """(signatures, structs, constants) of a header's text: every sa_* prototype as name ->
    (restype, [argtypes]), every `typedef struct` as name -> ctypes.Structure class (fields in the
    header's order), every integer #define SA_* and enumerator as name -> int.  A declaration the
    type rule does not cover raises NativeError naming it: nothing is guessed or skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, structs, signatures = {}, {}, {}

    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SA_\w+)[ \t]*(.*)$", text, flags=re.M):
        try:
            constants[name] = int(value.strip(), 0)
        except ValueError:
            raise NativeError(f"{_H}: #define {name} {value.strip()} is not an integer") from None
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def enum(m):
        nxt = 0
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, _, value = (s.strip() for s in item.partition("="))
            try:
                nxt = int(value, 0) if value else nxt
            except ValueError:
                raise NativeError(f"{_H}: enumerator `{item}` is not an integer") from None
            constants[name] = nxt
            nxt += 1
        return " "
    text = re.sub(r"\benum\s*\w*\s*\{([^{}]*)\}\s*;", enum, text)

    def struct(m):
        fields = []
        for line in filter(None, (s.strip() for s in m.group(1).split(";"))):
            head = _DECL.match(line)
            for d in line[head.end(1):].split(",") if head else [""]:
                dm = _DECLARATOR.fullmatch(d.strip())
                if dm is None:
                    raise NativeError(f"{_H}: cannot type `{line}` of {m.group(2)}")
                fname = dm.group(2) + ("_" if keyword.iskeyword(dm.group(2)) else "")
                fields.append((fname, _ctype(head.group(1), dm.group(1), f"{line}` of `{m.group(2)}")))
        structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": fields})
        return " "
    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)

    text, nopen = re.subn(r'\bextern\s+"C"\s*\{', " ", text)
    if "{" in text or text.count("}") != nopen:
        raise NativeError(f"{_H}: a braced block is neither an enum nor a typedef struct")
    for stmt in filter(None, (" ".join(s.split()) for s in text.replace("}", " ").split(";"))):
        m = re.fullmatch(r"(.*?)\b(sa_\w+) ?\(([^()]*)\)", stmt)
        if m is None:
            raise NativeError(f"{_H}: `{stmt}` is not an sa_* prototype")
        ret = " ".join(m.group(1).replace("*", " * ").split())
        if ret == "const char *":
            restype = ctypes.c_char_p
        elif ret == "void":
            restype = None
        elif ret in _SCALAR:
            restype = _SCALAR[ret]
        else:
            raise NativeError(f"{_H}: cannot type the return of `{stmt}`")
        argtypes = []
        for arg in ([] if m.group(3).strip() in ("", "void") else m.group(3).split(",")):
            am = _DECL.fullmatch(arg.strip())
            if am is None:
                raise NativeError(f"{_H}: cannot type `{arg.strip()}` of {m.group(2)}")
            argtypes.append(_ctype(am.group(1), am.group(2), f"{arg.strip()}` of `{m.group(2)}"))
        signatures[m.group(2)] = (restype, argtypes)

    for name in structs:   # every struct has a size check at load time (_check_abi)
        if _struct_id(name) not in constants:
            raise NativeError(f"{_H}: struct {name} has no {_struct_id(name)} for sa_struct_size")
    return signatures, structs, constants


def _read_header() -> str:
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise NativeError(f"{HEADER} is missing: the bindings are read from it ({e})") from None


# SIGNATURES: name -> (restype, argtypes); STRUCTS: SaWinoProblem, SaGateEpilogue, SaResampleJob,
# SaFeatureGateJob, SaLossMap (each also a name of this module); CONST: SA_* -> int
SIGNATURES, STRUCTS, CONST = parse_header(_read_header())
globals().update(STRUCTS)
# the library must be built from the same header as these bindings (the struct arrays are read at
# the library's stride)
ABI_VERSION = CONST["SA_ABI_VERSION"]

KERNEL_IDS = {
    "corr_volume_pyramid": 0, "corr_lookup": 1, "mono_masked_volume": 2, "softargmin_conf": 3,
    "weighted_lsq": 4, "gru_zr": 5, "gru_out": 6, "convex_upsample": 7, "misc": 8, "conv3d_fused": 9,
    "norm_act": 10, "conv2d_wino": 11, "conv2d_direct": 12, "conv2d_wino4": 13, "corr_shear": 14,
    "mono_pyramid": 15, "gru_plumbing": 16, "conv2d_small": 17, "conv2d_narrow": 18, "conv1x1": 19,
}

_lib: Optional[ctypes.CDLL] = None


def build(verbose: bool = False) -> str:
    """Compile libsa_hip.so for gfx950 with hipcc (via the repo Makefile)."""
    cmd = ["make", "-C", ROOT, "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise NativeError(f"building libsa_hip.so failed:\n{res.stdout}\n{res.stderr}")
    if verbose:
        print(res.stdout)
    return LIB_PATH


_USAGE_FIELDS = {"vgprs": r" VGPRs: (\d+)", "agprs": r" AGPRs: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)",
                 "lds": r"LDS Size \[bytes/block\]: (\d+)", "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)"}


def resource_usage(source_name: str, workdir, extra=()) -> dict:
    """{mangled kernel name: {"vgprs", "agprs", "scratch", "lds", "occupancy"}} of one csrc/*.hip
    source, from the resource-usage remarks of the product compile: the Makefile's own line for
    that source (per-file flags included, plus `extra`), with the object written into workdir."""
    stem = os.path.splitext(os.path.basename(source_name))[0]
    target = f"build/{stem}.o"
    dry = subprocess.run(["make", "-n", "-B", "-C", ROOT, target], capture_output=True, text=True)
    lines = [shlex.split(ln) for ln in dry.stdout.splitlines()]
    lines = [c for c in lines if "-c" in c and c[-2:] == ["-o", target]]
    if dry.returncode != 0 or len(lines) != 1:
        raise NativeError(f"make -n {target} gave no compile line:\n{dry.stdout}\n{dry.stderr}")
    cmd = lines[0][:-1] + [os.path.join(str(workdir), f"{stem}.o"), "-Rpass-analysis=kernel-resource-usage", *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    if res.returncode != 0:
        raise NativeError(f"{' '.join(cmd)} failed:\n{res.stderr[-2000:]}")
    out, cur = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        for key, pat in _USAGE_FIELDS.items():
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: the HIP hot path has no fallback. Build it with `make` "
                "or stereoanywhere_amd._native.build().")
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name, None)
            if fn is None:
                if os.environ.get("SA_HIP_LIB"):   # an older library of an A/B run: bind what it has
                    continue
                raise NativeError(f"{LIB_PATH} does not export {name}")
            fn.restype = res
            fn.argtypes = args
        _check_abi(h)
        _lib = h
    return _lib


def _check_abi(h) -> None:
    if not hasattr(h, "sa_abi_version"):
        if os.environ.get("SA_HIP_LIB"):   # an older library of an A/B run
            return
        raise NativeError(f"{LIB_PATH} has no sa_abi_version: rebuild it (`make`)")
    v = int(h.sa_abi_version())
    if v != ABI_VERSION:
        raise NativeError(f"{LIB_PATH} implements ABI version {v}, these bindings {ABI_VERSION}: rebuild it")
    for name, st in STRUCTS.items():
        got = int(h.sa_struct_size(CONST[_struct_id(name)]))
        if got == -1 and os.environ.get("SA_HIP_LIB"):   # an older library of an A/B run has no such struct
            continue
        if got != ctypes.sizeof(st):
            raise NativeError(f"{LIB_PATH}: {name} is {got} bytes in the library, "
                              f"{ctypes.sizeof(st)} in the bindings")


def call(name: str, *args) -> None:
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        msg = lib().sa_last_error().decode(errors="replace")
        raise NativeError(f"{name} failed ({rc}): {msg}")


def timing_enable(on: bool) -> None:
    call("sa_timing_enable", 1 if on else 0)


def timing_read(kernel: str):
    """(total_ms, launches) of one kernel since timing_enable / the last read."""
    ms = ctypes.c_double()
    n = ctypes.c_long()
    call("sa_timing_read", KERNEL_IDS[kernel], ctypes.byref(ms), ctypes.byref(n))
    return ms.value, n.value
