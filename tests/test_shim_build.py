"""tests/shim_build.py, the one builder of the tests' own artefacts: its staleness rule on temporary files, that it knows every
shim and check program of tests/host_shim and tests/device_shim, that no program reads a header from outside the directories
the rule watches (the compiler's own -MM says what each one reads), and the stand-alone check of unit_host.h under the host
sanitizers."""
import glob
import os

import pytest

import shim_build
from shim_build import DEVICE, HOST, ROOT

HOST_PROGRAMS = sorted([shim_build.host_shim_source(n) for n in shim_build.HOST_SHIMS] + [os.path.join(HOST, c) for c in shim_build.CHECKS])


def _touch(path, t):
    open(path, "a").close()
    os.utime(path, (t, t))


def test_staleness_rule(tmp_path):
    a, b = tmp_path / "csrc", tmp_path / "include"
    a.mkdir(); b.mkdir()
    dirs = (str(a), str(b))
    src, target, h1, h2, other = str(tmp_path / "x.cpp"), str(tmp_path / "libx.so"), str(a / "one.h"), str(b / "two.h"), str(b / "notes.txt")
    for f in (src, h1, h2):
        _touch(f, 1000)
    assert shim_build.stale(target, src, dirs)                      # missing
    _touch(target, 1000)
    assert not shim_build.stale(target, src, dirs)                  # as old as all of them: the stamp of a compile that started then
    _touch(target, 2000)
    assert not shim_build.stale(target, src, dirs)
    _touch(src, 3000)
    assert shim_build.stale(target, src, dirs)                      # older than the source
    _touch(src, 1000)
    for h in (h1, h2):
        _touch(h, 3000)
        assert shim_build.stale(target, src, dirs), h               # older than one header of a watched directory
        _touch(h, 1000)
    _touch(other, 3000)
    assert not shim_build.stale(target, src, dirs)                  # not a header
    assert sorted(shim_build.headers(dirs)) == [h1, h2]


def test_every_program_is_known_to_the_builder():
    on_disk = glob.glob(os.path.join(HOST, "*_shim.*")) + glob.glob(os.path.join(HOST, "*_check.cpp"))
    assert sorted(on_disk) == sorted(set(HOST_PROGRAMS))
    assert sorted(glob.glob(os.path.join(DEVICE, "*.hip"))) == sorted(os.path.join(DEVICE, d) for d in shim_build.DEVICE_SHIMS)
    # and every one of them is used: a test names the shim or the program it loads or runs
    tests = "".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "tests", "test_*.py")))
    for name in shim_build.HOST_SHIMS:
        assert 'host_shim("%s")' % name in tests, name
    for name in list(shim_build.CHECKS) + list(shim_build.DEVICE_SHIMS):
        assert '("%s", ' % name in tests, name


@pytest.mark.parametrize("source", HOST_PROGRAMS, ids=[os.path.basename(s) for s in HOST_PROGRAMS])
def test_every_header_read_lies_in_a_watched_directory(source):
    deps = shim_build.dependencies(source)
    assert os.path.realpath(source) in deps and len(deps) > 1
    watched = [os.path.realpath(d) for d in shim_build.WATCHED]
    for d in deps:
        assert d == os.path.realpath(source) or (d.endswith(".h") and os.path.dirname(d) in watched), d


def test_watched_directories_cover_the_device_shims():
    """the device compiles write no depfile, so follow the #include lines: every quoted header resolves into a watched directory"""
    import re
    watched = [os.path.realpath(d) for d in shim_build.WATCHED]
    todo, seen = [os.path.join(DEVICE, d) for d in shim_build.DEVICE_SHIMS], set()
    while todo:
        f = todo.pop()
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f).read(), re.M):
            h = os.path.realpath(os.path.join(os.path.dirname(f), inc))
            assert os.path.exists(h) and os.path.dirname(h) in watched and h.endswith(".h"), (f, inc)
            if h not in seen:
                seen.add(h)
                todo.append(h)
    assert os.path.realpath(os.path.join(shim_build.CSRC, "msm_reduce_kernels.h")) in seen


def test_unit_host_check_runs_clean_under_the_sanitizers(tmp_path):
    """tests/host_shim/unit_host_check.cpp: the argument checks of unit_host.h and PhaseTimer::copy_out as a program of its own,
    the host half built through hipcc with the sanitizers behind -Xarch_host"""
    out = shim_build.sanitized_check("unit_host_check.cpp", str(tmp_path / "unit_host_check"))
    assert out.returncode == 0 and (out.stdout + out.stderr).strip().endswith("ok"), (out.stdout + out.stderr)[-2000:]
