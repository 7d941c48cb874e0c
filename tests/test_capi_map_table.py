"""capi.MAP_ENTRY_POINTS, the one table both libraries' voxel-map argtypes come from, against the declarations of
include/madicp_hip.h and include/madicp_host.h: every row has a prototype on both sides with as many parameters as the argtypes the
table gives that side, and every map entry point either header declares is a row — one added to one side only fails here by name.
And the documented names (host_map_*, Context.map_*), which are one-line delegations to the shared operations: each hands every
argument on under the right name.  No library is loaded, no GPU."""
import inspect
import os
import re

import pytest

from mad_icp_amd import capi

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
ROWS = ["%s/%s" % row[:2] for row in capi.MAP_ENTRY_POINTS]


def prototypes(header):
    """{name: number of parameters} of the map functions a header declares"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    found = re.findall(r"^(?:int|void)\s+(madicp_(?:host_)?map_\w+)\s*\(([^;{]*)\)\s*;", text, flags=re.M)
    assert len(found) == len(set(name for name, _ in found)), "declared twice"
    return {name: len(params.split(",")) for name, params in found}


DEVICE, HOST = prototypes("madicp_hip.h"), prototypes("madicp_host.h")


def test_the_headers_were_read():
    assert len(DEVICE) >= 20 and len(HOST) >= 20 and all(n >= 1 for n in list(DEVICE.values()) + list(HOST.values()))
    assert DEVICE["madicp_map_size"] == 3 and HOST["madicp_host_map_size"] == 2 and HOST["madicp_host_map_destroy"] == 1
    assert not set(DEVICE) & set(HOST)


@pytest.mark.parametrize("row", range(len(ROWS)), ids=ROWS)
def test_row_has_both_prototypes_with_the_tables_parameter_counts(row):
    device_name, host_name = "madicp_map_" + capi.MAP_ENTRY_POINTS[row][0], "madicp_host_map_" + capi.MAP_ENTRY_POINTS[row][1]
    assert device_name in DEVICE, device_name + " is not declared in include/madicp_hip.h"
    assert host_name in HOST, host_name + " is not declared in include/madicp_host.h"
    assert len(capi.map_argtypes(device=True)[device_name]) == DEVICE[device_name], device_name
    assert len(capi.map_argtypes(device=False)[host_name]) == HOST[host_name], host_name


# the documented names that delegate to an operation of a made map: (function, the class it goes through, operation, leading handles)
DOCUMENTED = [(f, capi.HostMap, name[len("host_map_"):], 1) for name, f in sorted(vars(capi).items()) if name.startswith("host_map_")]
DOCUMENTED += [(f, capi.DeviceMap, name[len("map_"):], 2) for name, f in sorted(vars(capi.Context).items()) if name.startswith("map_")]
DOCUMENTED = [d for d in DOCUMENTED if not d[2].startswith("create")]  # (those are HostMap.create / DeviceMap.create: every map suite)
OTHER_NAME = {"insert_cloud": "insert", "insert_attr": "insert", "register_cloud": "register", "destroy": "close", "release": "close"}
NO_ANSWER = ("track_removed", "clear", "destroy", "release")


@pytest.mark.parametrize("wrapper,cls,op,handles", DOCUMENTED, ids=[d[0].__qualname__ for d in DOCUMENTED])
def test_documented_name_hands_every_argument_to_the_shared_operation(monkeypatch, wrapper, cls, op, handles):
    """host_map_X(h, ...) and Context.map_X(mid, ...) called with one distinct value per parameter: the shared operation gets each
    value under the parameter of the same name (the scan under `scan`, insert_attr's words behind t), and its answer comes back"""
    method = OTHER_NAME.get(op, op)
    takes = inspect.signature(getattr(cls, method))
    seen = {}

    def shared(self, *a, **k):
        seen.update(takes.bind(self, *a, **k).arguments)
        return "answer"

    monkeypatch.setattr(cls, method, shared)
    values = {n: object() for n in inspect.signature(wrapper).parameters}
    assert wrapper(*values.values()) == (None if op in NO_ANSWER else "answer")
    given = dict(list(values.items())[handles:])  # (behind h, or behind self and mid)
    assert seen.pop("attr", ()) == ((given.pop("attr"),) if op == "insert_attr" else ())
    del seen["self"]
    assert seen == {("scan" if n in ("xyz", "cid") else n): v for n, v in given.items()}


def test_every_declared_map_entry_point_is_a_row():
    assert sorted(set(DEVICE) - set(capi.map_argtypes(device=True))) == []
    assert sorted(set(HOST) - set(capi.map_argtypes(device=False))) == []
    assert sorted(set(capi.map_argtypes(device=True)) - set(DEVICE)) == [] and sorted(set(capi.map_argtypes(device=False)) - set(HOST)) == []
