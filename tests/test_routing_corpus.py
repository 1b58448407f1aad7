"""The routing corpus (tests/routing_corpus.py): every plan x row count x launch flag x routing switch gets the kernels
that were recorded for it.  `hdk_hip_describe_launch` prints the route that `hdk_hip_launch` launches (csrc/route.h), so this
pins what runs, on a CPU-only box.  The table was recorded before the routing step existed, from the launch description of
that time; the rows where that description disagreed with its launch (a projection under FORCE_SCALAR: described as the
batched interpreter, run on hdk_scan_project_scalar) were edited to what the launch ran."""
import json
import os
import re

import pytest

import routing_corpus as RC


@pytest.fixture(scope="module")
def golden():
    with open(RC.GOLDEN) as f:
        return json.load(f)


def test_every_combination_routes_as_recorded(golden):
    want = RC.unpack(golden)
    got = RC.describe_all(RC.corpus())
    assert tuple(golden["variants"]) == RC.VARIANTS and tuple(golden["rows"]) == RC.ROWS
    assert list(got) == list(want)
    wrong = [(pid, rows, v, got[pid][ri][v], want[pid][ri][v]) for pid in want for ri, rows in enumerate(RC.ROWS) for v in RC.VARIANTS
             if got[pid][ri][v] != want[pid][ri][v]]
    assert not wrong, (len(wrong), wrong[:10])


def test_every_route_is_in_the_corpus(golden):
    """every enumerator of csrc/route.h's table is some row's answer (a clustering pre-pass in front of it or not)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hdk_amd", "csrc", "route.h")
    with open(path) as f:
        text = f.read()
    text = text[text.index("#define HDK_ROUTE_LIST(X)"):text.index("enum RouteKind")]
    text = re.sub(r"/\*.*?\*/", "", text.replace("\\\n", " "), flags=re.S)
    routes = {name: "".join(re.findall(r'"([^"]*)"', lits)) for name, _family, lits in re.findall(r'X\((\w+),\s*(\w+),\s*((?:"[^"]*"\s*)+)\)', text)}
    assert len(routes) >= 39 and len(set(routes.values())) == len(routes)
    seen = {n.replace("hdk_cluster_by_key,hdk_cluster_params,", "") for n in golden["names"]}
    assert seen == set(routes.values()), (sorted(set(routes.values()) - seen), sorted(seen - set(routes.values())))
    assert any(n.startswith("hdk_cluster_by_key,hdk_cluster_params,") for n in golden["names"])
