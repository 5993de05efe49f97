"""orc_amd/build.py decides what to compile again from each object's
dependency file (the compiler's -MD output). The rule, on temporary files:
nothing is compiled here."""
import os

from orc_amd.build import stale


def test_an_object_is_stale_by_its_own_dependencies(tmp_path):
    src, hdr, other, tool = (str(tmp_path / n) for n in ("unit.hip", "unit.hh", "other.hh", "build.py"))
    obj, dep = str(tmp_path / "unit.hip.o"), str(tmp_path / "unit.hip.o.d")

    def at(path, t, text=""):  # write `path`, last modified at second t
        with open(path, "w") as f:
            f.write(text)
        os.utime(path, (t, t))

    def fresh():
        for p in (src, hdr, other, tool):
            at(p, 1000)
        at(dep, 2000, "%s: %s \\\n  %s\n" % (obj, src, hdr))  # make syntax, as the compiler writes it
        at(obj, 2000)

    check = lambda: stale(obj, src, dep, tools=(tool,))
    fresh()
    assert not check()  # a fresh object
    at(other, 3000)
    assert not check()  # a header no dependency file names is nobody's business
    at(src, 3000)
    assert check()  # a touched source
    fresh()
    at(hdr, 3000)
    assert check()  # a touched file that only the dependency file names
    fresh()
    at(tool, 3000)
    assert check()  # the build script itself
    fresh()
    os.remove(dep)
    assert check()  # no dependency file yet
    fresh()
    os.remove(hdr)
    assert check()  # the dependency file names a file that no longer exists
    fresh()
    os.remove(obj)
    assert check()
