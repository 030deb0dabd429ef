"""The batched delta records through the Node host: the addon's getDeltasBatch equals the Python binding's on one small
legacy-format batch (and its own per-document getDeltas), and BatchReplayEngine's catch-up blobs, resolved from one
batched call, equal those of the per-document path.  The script gathers, this test compares."""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]


def _msg(client, op, seq, ref, msn=0):
    return {"clientId": client, "sequenceNumber": seq, "referenceSequenceNumber": ref, "minimumSequenceNumber": msn,
            "type": "op", "contents": op}


def _docs():
    ins = lambda p, s: {"type": 0, "pos1": p, "seg": s}  # noqa: E731
    docs = []
    for n in (1, 66, 0):  # lagging messages per document: 1 record, 66 (a second round), none
        msgs = [_msg("w", ins(0, "base text"), 1, 0)]
        for k in range(n):
            # (the first one, at referenceSequenceNumber 0, sees an empty view: position 0; the others see the base)
            op = ins(k % 5 if k else 0, "ab"[k % 2]) if k % 3 != 2 else {"type": 1, "pos1": 2, "pos2": 3}
            msgs.append(_msg("v", op, k + 2, 0 if k == 0 else k))
        if n == 0:
            msgs.append(_msg("w", ins(2, "--"), 2, 1))
        docs.append({"observer": "me", "msgs": msgs})
    return docs


def test_addon_equals_python_binding_and_per_document_path(tmp_path):
    from fluidframework_amd import build
    from fluidframework_amd.batch import Interner, build_batch
    from fluidframework_amd.engine import Engine
    from fluidframework_amd.sequence import SequenceLog

    if build.build_node_addon() is None:
        pytest.skip("node headers missing")
    docs = _docs()
    f = tmp_path / "docs.json"
    f.write_text(json.dumps(docs))
    r = subprocess.run(["node", os.path.join(HERE, "node", "deltas_batch_engine.js"), str(f)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout)
    assert res["enumerable"] is False, "the addon's new function must not join its enumerable exports"

    # the Python binding on the same messages
    it = Interner()
    logs = []
    for d in docs:
        log = SequenceLog(legacy=True)
        log.start_collab(d["observer"])
        for m in d["msgs"]:
            log.message(dict(m), it)
        logs.append(log)
    n = len(docs) + 1
    eng = Engine(n, snapshot_v1=False, max_segments=1024, heap_entries=1024, text_units=1 << 12, prop_words=1 << 10,
                 remover_cells=1 << 10)
    eng.apply(build_batch(logs, it))
    first, recs, poff, words = eng.deltas_batch(n=n, props=True)
    singles = [eng.deltas(d) for d in range(n)]
    assert [len(s) for s in singles] == [1, len(singles[1]), 0, 0] and len(singles[1]) >= 66
    flat = lambda a: a.view("<i4").reshape(-1).tolist()  # noqa: E731
    assert res["all"]["docFirst"] == first.tolist() and res["all"]["records"] == flat(recs)
    assert res["all"]["propsOff"] == poff.tolist() and res["all"]["props"] == words.tolist()
    assert res["singles"] == [flat(s) for s in singles]
    order = res["order"]
    assert res["listed"]["docFirst"] == np.cumsum([0] + [len(singles[d]) for d in order]).tolist()
    assert res["listed"]["records"] == [w for d in order for w in flat(singles[d])]
    assert "propsOff" not in res["listed"] and "props" not in res["listed"]
    assert res["host"]["records"] == flat(singles[1]) + flat(singles[0])

    # the catch-up blobs: one batched call after the run against a getDeltas call per document, and the Python host's
    assert res["catchup"] == res["catchupPerDocument"]
    for log, d in zip(logs, range(len(docs))):
        log.resolve(singles[d])
    want = [log.catchup_blob() for log in logs]
    assert [None if c is None else base64.b64decode(c) for c in res["catchup"]] == want
    assert want[0] and want[1]
    eng.close()
