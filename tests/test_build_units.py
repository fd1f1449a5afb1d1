"""The table of kernel families in __graft_entry__.py against itself and against the lists of algames_kernels.hpp (read as text): which
configurations exist, in which translation unit, built with which flags.  No compiler, no GPU."""
import os
import re

import __graft_entry__ as ge

HEADER = os.path.join(ge.CSRC, "algames_kernels.hpp")


def _header_lists():
    """{name: (parameters, body)} of every #define ALG_CFGS_* of the header, continuation lines joined"""
    txt = open(HEADER).read().replace("\\\n", " ")
    return {m.group(1): ([p.strip() for p in m.group(2).split(",")], m.group(3).strip())
            for m in re.finditer(r"^#define\s+(ALG_CFGS_\w+)\(([^)]*)\)(.*)$", txt, flags=re.M)}


def _is_composite(body):
    """nothing but other one-parameter lists, e.g. ALG_CFGS_EXT(X) = ALG_CFGS_EXT_DI(X) ALG_CFGS_EXT_UNI(X) ..."""
    return re.fullmatch(r"(ALG_CFGS_\w+\(X\)\s*)+", body) is not None


def _leaves(lists, name):
    params, body = lists[name]
    assert params == ["X"], name
    if not _is_composite(body):
        return [name]
    return [leaf for part in re.findall(r"(ALG_CFGS_\w+)\(X\)", body) for leaf in _leaves(lists, part)]


def _table_names():
    names = {"ALG_CFGS_ONE"}
    for f in ge.FAMILIES:
        names |= {f.cfgs} | {c for _, c in ge._halves(f)} | ({f.handoff} if f.handoff else set())
    return names


def _family_units(f):
    return ge._kernel_units(f) + ge._sched_units(f) + ge._kkt_units(f)


def test_stems_are_unique_and_every_source_exists():
    stems = [u[1] for u in ge.HIP_UNITS]
    assert len(stems) == 76 and len(set(stems)) == 76
    for src, stem, extra in ge.HIP_UNITS:
        assert os.path.exists(os.path.join(ge.CSRC, src)), (stem, src)
    # HIP_DEPS lists every source and header of csrc/, and the C header
    on_disk = {os.path.join(ge.CSRC, f) for f in os.listdir(ge.CSRC) if f.endswith((".hip", ".hpp"))}
    assert on_disk <= set(ge.HIP_DEPS) and all(os.path.exists(d) for d in ge.HIP_DEPS)
    assert os.path.join(ge.ROOT, "include", "algames_hip.h") in ge.HIP_DEPS


def test_the_ext_defines_default_to_the_base_lists():
    """a command line that names only the entry (tests/probes of an older tree, a hand-written hipcc line) builds the ext = 0 unit it always
    built, instead of failing -- the variant build of tests/test_gpu_refinement.py relies on its unit compiling"""
    for src, name in (("algames_base.hip", "ALG_BASE_EXT"), ("algames_mw.hip", "ALG_MW_EXT")):
        txt = open(os.path.join(ge.CSRC, src)).read()
        assert re.search(r"#ifndef %s\n#define %s 0\b" % (name, name), txt), src
    assert ["-DALG_BASE_EXT=0"] * 9 == [u[2][1] for u in ge.HIP_UNITS if u[1].startswith("algames_base_") and "scen" not in u[1]]
    assert ("algames_mw.hip", "algames_mw", ["-DALG_MW_EXT=0"]) in ge.HIP_UNITS


def test_the_unit_counts_per_kernel_set():
    n = {k: len(v) for k, v in ge.KERNEL_SETS.items()}
    assert n == {"host": 1, "kernels": 18 + 14 + 3, "sched": 21, "plant": 1, "kkt": 18}
    assert sum(n.values()) == 76 == len(ge.HIP_UNITS)
    base = [u for u in ge.KERNEL_SETS["kernels"] if u[0] == "algames_base.hip"]
    team = [u for f in ge.FAMILIES if f.team for u in ge._kernel_units(f)]
    assert len(base) == 18 and len(team) == 3 and len(ge.KERNEL_SETS["kernels"]) - len(base) - len(team) == 14
    # kernels, scheduled loop and KKT solve for a one-wavefront family; kernels and scheduled loop for a team
    for f in ge.FAMILIES:
        assert ge._kernel_units(f) and ge._sched_units(f) and bool(ge._kkt_units(f)) == (not f.team), f.name
        # the base lists split into their halves for the scheduled loops and the KKT solves
        assert len(ge._sched_units(f)) == (2 if f.ext is not None and not f.team else 1), f.name
    assert [u[1] for u in ge.KERNEL_SETS["kernels"]][:18] == ["algames_base_%d" % k for k in range(9)] + ["algames_base_scen_%d" % k for k in range(9)]
    assert {"algames_hip", "algames_mw", "algames_mw_scen", "algames_plant", "algames_sched_ext_di", "algames_kkt_p7"} <= {u[1] for u in ge.HIP_UNITS}


def test_every_family_has_one_flag_class_and_every_unit_takes_it():
    assert len({f.name for f in ge.FAMILIES}) == len(ge.FAMILIES) == len({f.cfgs for f in ge.FAMILIES})
    assert set(ge.FLAG_CLASSES) == {"tile", "dense", "dense_nolso"}
    assert ge.FLAG_CLASSES == {"tile": ge.HIP_FLAGS_TILE, "dense": ge.HIP_FLAGS_DENSE, "dense_nolso": ge.HIP_FLAGS_DENSE + ge.HIP_FLAGS_NOLSO}
    seen = {}
    for f in ge.FAMILIES:
        assert f.flags in ge.FLAG_CLASSES, f
        for u in _family_units(f):
            assert u[1] not in seen, (u[1], f.name, seen.get(u[1]))            # a unit belongs to one family
            seen[u[1]] = f.name
            assert ge.compile_flags(u) == ge.HIP_FLAGS + ge.FLAG_CLASSES[f.flags] + u[2], u[1]
    # the two units outside the families: the host code and the plant knots of all one-wavefront families
    outside = [u for u in ge.HIP_UNITS if u[1] not in seen]
    assert sorted(u[1] for u in outside) == ["algames_hip", "algames_plant"]
    for u in outside:
        assert ge.compile_flags(u) == ge.HIP_FLAGS + ge.HIP_FLAGS_TILE + u[2], u[1]
    assert len(seen) + len(outside) == 76
    # the load/store optimizer stays on in the dense class except for the two quadrotor lists
    assert sorted(f.cfgs for f in ge.FAMILIES if f.flags == "dense_nolso") == ["ALG_CFGS_QUAD", "ALG_CFGS_QUAD_EXT"]
    assert [f.flags for f in ge.FAMILIES if f.cfgs == "ALG_CFGS_DI1"] == ["dense"]


def test_every_list_the_table_names_is_defined_in_the_header():
    lists = _header_lists()
    for name in sorted(_table_names()):
        assert name in lists and lists[name][0] == ["X"], name
    # ... and so is everything a command line names
    for src, stem, extra in ge.HIP_UNITS:
        for d in extra:
            m = re.fullmatch(r"-DALG_UNIT_CFGS=(\w+)", d)
            assert m is None or m.group(1) in _table_names(), (stem, d)
            m = re.fullmatch(r"-DALG_UNIT_KERNELS=(\w+)", d)
            assert m is None or re.search(r"^#define\s+%s\(" % m.group(1), open(HEADER).read(), flags=re.M), (stem, d)


def test_every_leaf_list_of_the_header_is_named_by_the_table():
    """what catches a family added in one place only"""
    lists = _header_lists()
    leaves = {name for name, (params, body) in lists.items() if params == ["X"] and not _is_composite(body)}
    assert len(leaves) >= 23, sorted(leaves)                 # (the text scan found them: 19 families, two of them in halves, two hand-off lists)
    assert leaves <= _table_names(), sorted(leaves - _table_names())
    # every family's units instantiate leaves, each leaf in one family
    owner = {}
    for f in ge.FAMILIES:
        for leaf in _leaves(lists, f.cfgs):
            assert leaf not in owner, (leaf, f.name, owner.get(leaf))
            owner[leaf] = f.name
        assert [l for _, c in ge._halves(f) for l in _leaves(lists, c)] == _leaves(lists, f.cfgs), f.name
    handoff = {f.handoff for f in ge.FAMILIES if f.handoff}
    assert set(owner) | handoff == leaves
    # the host's list of one-wavefront configurations is the one-wavefront families, no more and no less
    assert sorted(_leaves(lists, "ALG_CFGS_ONE")) == sorted(l for f in ge.FAMILIES if not f.team for l in _leaves(lists, f.cfgs))
    assert len(_leaves(lists, "ALG_CFGS_ONE")) == len(set(_leaves(lists, "ALG_CFGS_ONE")))
    # the twins are their E = 0 lists with another ext column, not copies
    for a, b in (("ALG_CFGS_BASE_DI", "ALG_CFGS_BASE_SCEN_DI"), ("ALG_CFGS_BASE_UNI", "ALG_CFGS_BASE_SCEN_UNI"), ("ALG_CFGS_MW", "ALG_CFGS_MW_SCEN"),
                 ("ALG_CFGS_HANDOFF", "ALG_CFGS_HANDOFF_SCEN")):
        assert lists[a][1].endswith("_E(X, 0)") and lists[b][1] == lists[a][1].replace("(X, 0)", "(X, 2)"), (a, b)
    for f in ge.FAMILIES:
        if f.ext is not None:
            assert all(lists[l][1].endswith("_E(X, %d)" % f.ext) for l in _leaves(lists, f.cfgs)), f.name
            assert f.handoff is None or lists[f.handoff][1].endswith("_E(X, %d)" % f.ext), f.name
