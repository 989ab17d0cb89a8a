"""The dependency lists of the build recipe (psdr_jit_amd/build.py::hip_units) against the include graph of the sources.

An object is compiled again when the signature over its source, its dependency list and its flags changes - not by modification times.
A header that a unit includes but its list forgets therefore means a stale binary: the edit never reaches the library the GPU tests load.
And the kernel units must not depend on api.hip: an edit of the host code would recompile (and run through the register allocator again)
eight units of device code that cannot see it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = re.compile(r'^\s*#\s*include\s*"([^"]+)"', re.M)


def _load_build():
    """by path: the recipe needs none of the package's native libraries"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_psdr_build_deps_t", os.path.join(ROOT, "psdr_jit_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _reachable(src):
    """every file a quoted #include reaches from `src`, transitively"""
    seen, todo = set(), [os.path.realpath(src)]
    while todo:
        f = todo.pop()
        with open(f) as fh:
            text = fh.read()
        for inc in INCLUDE.findall(text):
            p = os.path.realpath(os.path.join(os.path.dirname(f), inc))
            assert os.path.exists(p), "%s includes %s, which does not exist" % (os.path.relpath(f, ROOT), inc)
            if p not in seen:
                seen.add(p)
                todo.append(p)
    return seen


def test_every_included_header_is_in_its_units_dependency_list():
    b = _load_build()
    units = b.hip_units()
    assert len([u for u in units if u[0].startswith("tu")]) == b.N_KERNEL_UNITS
    assert {"main", "scene"} <= {u[0] for u in units}
    for name, src, _defs, deps in units:
        listed = {os.path.realpath(d) for d in deps}
        missing = sorted(os.path.relpath(p, ROOT) for p in _reachable(src) - listed)
        assert not missing, "unit %s (%s) includes %s, missing from its dependency list" % (name, os.path.relpath(src, ROOT), missing)
        # ... and the whole-library signature (the staleness check of the library and of tools/variants.py) covers the unit
        whole = {os.path.realpath(f) for f in b.HIP_SRCS + b.HIP_DEPS}
        assert ({os.path.realpath(src)} | listed) <= whole, "unit %s: %s not in HIP_SRCS + HIP_DEPS" % (name, sorted(({os.path.realpath(src)} | listed) - whole))


def test_the_operator_units_are_one_list_compiled_in_this_order():
    b = _load_build()
    names = [u[0] for u in b.hip_units()]
    order = ["precond", "adaptive", "denoise", "vdenoise", "subdiv", "msloss", "ssim", "meshreg", "chamfer", "sdf", "mtet", "latreg", "pointmesh"]
    assert [u[0] for u in b.OPERATOR_UNITS] == order
    assert names[names.index("scene") + 1:] == order          # after the host, kernel and scene units, and nothing after them


def test_no_kernel_unit_depends_on_the_host_source():
    b = _load_build()
    api = os.path.realpath(b.API_SRC)
    for name, src, _defs, deps in b.hip_units():
        if not name.startswith("tu"):
            continue
        inputs = {os.path.realpath(f) for f in [src] + list(deps)} | _reachable(src)
        assert api not in inputs, "kernel unit %s is compiled again whenever api.hip changes" % name
