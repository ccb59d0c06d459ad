"""MI355X (gfx950) build of the Stereo Anywhere cost-volume hot path.

Importing the package points MIOpen at the in-repo find/perf database (miopen_db/), so the
dense convolutions that stay on MIOpen use the algorithms measured on MI355X for these
shapes instead of immediate-mode heuristics; without entries MIOpen falls back to its
heuristics.  MIOpen rewrites its user database and its compiled-kernel cache while it runs, so
the process works on a copy of miopen_db/ under build/ (made once per content of the committed
files) and the committed files stay as they are.  Override with MIOPEN_USER_DB_PATH /
MIOPEN_CUSTOM_CACHE_DIR (compiled-kernel cache for the chosen solvers).  Regenerate with
`MIOPEN_USER_DB_PATH=miopen_db MIOPEN_CUSTOM_CACHE_DIR=miopen_db/cache bench.py --miopen-find 1`
on the box.
"""
import os as _os

_ROOT = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))
_DB = _os.path.join(_ROOT, "miopen_db")


def _working_db() -> str:
    """build/miopen_db-<hash of the committed files>: a copy of miopen_db/ for MIOpen to read and
    write.  Made in a temporary directory and renamed into place, so processes that start together
    (the ranks of a multi-GPU run) see either nothing or the whole copy.  Where the tree cannot
    be written, miopen_db/ itself."""
    import hashlib
    import shutil
    import tempfile

    h = hashlib.sha256()
    for dirpath, dirnames, filenames in _os.walk(_DB):
        dirnames.sort()
        for name in sorted(filenames):
            path = _os.path.join(dirpath, name)
            h.update(_os.path.relpath(path, _DB).encode())
            with open(path, "rb") as f:
                h.update(f.read())
    build = _os.path.join(_ROOT, "build")
    dst = _os.path.join(build, "miopen_db-" + h.hexdigest()[:12])
    if _os.path.isdir(dst):
        return dst
    try:
        _os.makedirs(build, exist_ok=True)
        tmp = tempfile.mkdtemp(dir=build, prefix=".miopen_db-")
    except OSError:
        return _DB
    try:
        shutil.copytree(_DB, _os.path.join(tmp, "db"))
        _os.makedirs(_os.path.join(tmp, "db", "cache"), exist_ok=True)
        _os.rename(_os.path.join(tmp, "db"), dst)
    except OSError:
        pass   # (another process renamed its copy into place first)
    shutil.rmtree(tmp, ignore_errors=True)
    return dst if _os.path.isdir(dst) else _DB


if _os.path.isdir(_DB) and not ("MIOPEN_USER_DB_PATH" in _os.environ and "MIOPEN_CUSTOM_CACHE_DIR" in _os.environ):
    _work = _working_db()
    _os.environ.setdefault("MIOPEN_USER_DB_PATH", _work)
    _os.environ.setdefault("MIOPEN_CUSTOM_CACHE_DIR", _os.path.join(_work, "cache"))
