"""The blob-id cache's life cycle through the Node host: BatchReplayEngine.blobCacheGeneration / blobCacheAges /
blobCacheTrim / blobCacheTrimTo / blobCacheExport / blobCacheImport.  The script runs a fixed sequence of calls -- a
trim that takes every other id out of two 300-entry probe chains, an export imported into a second engine, trims to a
cap -- and prints what the cache shows after every step; gitid.BlobCacheModel runs through the same sequence here."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
METHODS = ["blobCacheGeneration", "blobCacheAges", "blobCacheTrim", "blobCacheTrimTo", "blobCacheExport",
           "blobCacheImport"]


def test_addon_exposes_the_methods():
    node = os.path.join(ROOT, "fluidframework_amd", "node")
    native = open(os.path.join(node, "mtr_napi.cc")).read()
    index = open(os.path.join(node, "index.js")).read()
    types = open(os.path.join(node, "index.d.ts")).read()
    for name in METHODS:
        assert re.search(r'\{"%s", nullptr, [A-Za-z]+,' % name, native), name  # registered with the addon
        assert re.search(r"^    %s\(" % name, index, re.M), name  # a method of BatchReplayEngine
        assert "native().%s(this.h" % name in index, name
        assert re.search(r"^\t%s\(" % name, types, re.M), name


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")
def test_trim_export_and_import(tmp_path):
    from test_blob_cache_trim import _colliding_ids, _hex

    from fluidframework_amd import build
    from fluidframework_amd.gitid import BlobCacheModel

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    ids = _hex(_colliding_ids())
    arg = tmp_path / "ids.json"
    arg.write_text(json.dumps(ids))
    r = subprocess.run(["node", os.path.join(HERE, "node", "blob_cache_trim_engine.js"), str(arg)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    steps = {s["name"]: s for s in res["steps"]}
    assert len(steps) == len(res["steps"]) == 10

    def same(name, model, removed=None):
        s = steps[name]
        assert (s["size"], s["generation"]) == (model.size(), model.generation), name
        assert (s["ids"], s["ages"]) == model.export(), name
        assert s["ages4"] == model.ages(4) and s["has"] == model.has(ids), name
        assert s.get("removed") == removed, name

    even, odd = ids[::2], ids[1::2][::-1]
    a = BlobCacheModel()
    same("empty", a)
    a.add(even)
    a.import_(ids[:1], [1])
    a.add(odd)
    same("two generations", a)
    assert a.size() == 600 and a.generation == 1
    same("trim", a, a.trim(1))
    assert a.ids() == odd  # every survivor of both chains is found, no removed id is (`has` above)
    a.add([ids[4]])
    same("a removed id again", a)
    assert a.ids()[-1] == ids[4]
    a.import_(even[:50], [2 + k % 3 for k in range(50)])
    same("older entries", a)
    b = BlobCacheModel()
    b.import_(*a.export())
    same("imported", b)
    assert b.export() == a.export() and b.generation == a.generation == 4
    same("imported nothing", b)
    same("trim to 320", b, b.trim_to(320))
    assert b.size() == 17  # (generation 1 does not fit whole: it goes, and generation 0 with it)
    same("trim to 0", b, b.trim_to(0))
    assert b.size() == 0 and b.generation == 4
    same("the first engine", a)
    assert "1..1024" in res["refused"]
