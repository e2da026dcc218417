"""CPU: the library's stale check sees every file the library is compiled from.

_build.DEPS decides when libtkv_amq.so is rebuilt (source_digest).  A header that a unit includes
and DEPS does not list means a stale library after an edit, which nothing else would notice.
No device, no compiler."""
import os
import re
import shutil

from turtle_kv_amd import _build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
# where `#include "..."` looks: beside the including file, then the -I of _build.FLAGS
INCLUDE_DIRS = [f[2:] for f in _build.FLAGS if f.startswith("-I")]


def resolve(name, beside):
    for d in [os.path.dirname(beside), *INCLUDE_DIRS]:
        p = os.path.normpath(os.path.join(d, name))
        if os.path.exists(p):
            return p
    return None


def test_every_include_is_a_dep():
    deps = {os.path.normpath(p) for p in _build.DEPS}
    assert {os.path.normpath(p) for p in _build.SOURCES} <= deps
    seen, todo, edges = set(), [os.path.normpath(p) for p in _build.SOURCES], 0
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            text = f.read()
        for name in INCLUDE.findall(text):
            inc = resolve(name, path)
            assert inc is not None, f'{path}: #include "{name}" resolves to no file'
            assert inc in deps, f"{path} includes {inc}, which _build.DEPS does not list"
            edges += 1
            todo.append(inc)
    # (the walk did follow includes: the units share headers, and headers include headers)
    assert edges > len(_build.SOURCES) and len(seen) > len(_build.SOURCES) + 3


def test_digest_sees_every_csrc_header(tmp_path, monkeypatch):
    csrc = os.path.join(_build.HERE, "csrc")
    copy = tmp_path / "csrc"
    shutil.copytree(csrc, copy)
    headers = sorted(f for f in os.listdir(csrc) if f.endswith(".h"))
    assert headers
    moved = [str(copy / os.path.basename(p)) if os.path.dirname(p) == csrc else p for p in _build.DEPS]
    monkeypatch.setattr(_build, "DEPS", moved)
    before = _build.source_digest()
    for h in headers:
        with open(copy / h, "ab") as f:
            f.write(b"\n")
        after = _build.source_digest()
        assert after != before, f"{h}: a changed header leaves the digest as it was"
        before = after
