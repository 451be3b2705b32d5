"""The extension's staleness check sees everything the sources include.

No GPU and no compiler: the test reads the ``#include "…"`` lines of every
source ``ops.build`` compiles and drives ``_stale()`` on copies under
``tmp_path``.
"""

import os
import re
import shutil

from distributed_sigmoid_loss_amd.ops import build

LOCAL_INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.MULTILINE)


def local_includes(path):
    with open(path, encoding="utf-8") as f:
        return LOCAL_INCLUDE.findall(f.read())


def test_every_local_include_is_a_dependency():
    deps = {os.path.realpath(p) for p in build._deps()}
    assert {os.path.realpath(s) for s in build._SRCS} <= deps
    seen = set()
    for src in build._SRCS:
        for name in local_includes(src):
            inc = os.path.realpath(os.path.join(os.path.dirname(src), name))
            assert os.path.isfile(inc), f"{src} includes missing {name}"
            assert inc in deps, f"{name} (from {src}) is not a dependency"
            seen.add(inc)
    # the shared tile header is what this guards
    assert any(p.endswith("pair_tile.h") for p in seen)
    # headers may include headers
    for hdr in deps - {os.path.realpath(s) for s in build._SRCS}:
        for name in local_includes(hdr):
            inc = os.path.realpath(os.path.join(os.path.dirname(hdr), name))
            assert inc in deps, f"{name} (from {hdr}) is not a dependency"


def test_newer_header_makes_the_extension_stale(tmp_path, monkeypatch):
    kernels = tmp_path / "kernels"
    shutil.copytree(os.path.dirname(build._SRCS[0]), kernels)
    srcs = [str(kernels / os.path.basename(s)) for s in build._SRCS]
    so = tmp_path / "_siglip_hip.so"
    monkeypatch.setattr(build, "_SRCS", srcs)
    monkeypatch.setattr(build, "SO_PATH", str(so))

    assert build._stale()                      # no .so yet
    so.write_bytes(b"")
    headers = [p for p in build._deps() if p not in srcs]
    assert headers and all(p.startswith(str(kernels)) for p in headers)

    now = os.path.getmtime(so)
    for p in build._deps():
        os.utime(p, (now - 10, now - 10))
    assert not build._stale()
    for hdr in headers:
        os.utime(hdr, (now + 10, now + 10))
        assert build._stale(), f"{hdr} newer than the .so went unnoticed"
        os.utime(hdr, (now - 10, now - 10))
    assert not build._stale()
    os.utime(srcs[0], (now + 10, now + 10))
    assert build._stale()
