'use strict';
// The batched delta records through the Node host: the addon's getDeltasBatch against its per-document getDeltas on
// one small legacy-format batch, and BatchReplayEngine's catch-up blobs (resolved from one batched call after the run)
// against those of an engine whose _afterRun asks per document.
// Input: a JSON file [{observer, msgs: [ISequencedDocumentMessage...]}...].  Output: the addon's results as plain
// arrays and both engines' catchupOps blobs (base64).
// usage: node deltas_batch_engine.js <docs.json>
const fs = require('fs');
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const docs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const options = { snapshotV1: 0, maxSegments: 1024, heapEntries: 1024, textUnits: 1 << 12, propWords: 1 << 10,
    removerCells: 1024 };

function replay(perDocument) {
    const engine = new m.BatchReplayEngine(docs.length + 1, options);
    if (perDocument) {
        engine._afterRun = function () {
            this.catchUps.forEach((c, d) => { if (c.pending.length) c.resolve(m.native().getDeltas(this.h, d)); });
            this.dirty = false;
            this.summarized = false;
        };
    }
    const clients = docs.map((d) => {
        const c = engine.createClient();
        c.startOrUpdateCollaboration(d.observer);
        return c;
    });
    docs.forEach((d, i) => { for (const msg of d.msgs) clients[i].applyMsg(msg); });
    engine.flush();
    return { engine, clients };
}

// (summarize applies a batch of its own: call it after the delta records of the replayed batch were read)
function catchups(clients) {
    return docs.map((d, i) => {
        const last = d.msgs[d.msgs.length - 1];
        const s = clients[i].summarize({ deltaManager: { minimumSequenceNumber: last.minimumSequenceNumber,
            lastSequenceNumber: last.sequenceNumber } }, undefined, undefined, undefined);
        const b = s.summary.tree.catchupOps;
        return b ? Buffer.from(b.content, 'utf8').toString('base64') : null;
    });
}

const plain = (r) => {
    const o = {};
    for (const k of Object.keys(r)) o[k] = Array.from(r[k]);
    return o;
};
const a = replay(false);
const b = replay(true);
const n = docs.length + 1;  // (the last document is in no batch)
const native = m.native();
const order = [2, 0, n - 1, 2];
const res = {
    all: plain(native.getDeltasBatch(a.engine.h, null, n, true)),
    listed: plain(native.getDeltasBatch(a.engine.h, Uint32Array.from(order), order.length, false)),
    host: plain(a.engine.getDeltasBatch([a.clients[1], a.clients[0]], false)),
    order,
    singles: Array.from({ length: n }, (_, d) => Array.from(native.getDeltas(a.engine.h, d))),
    enumerable: Object.keys(native).includes('getDeltasBatch'),
};
res.catchup = catchups(a.clients);
res.catchupPerDocument = catchups(b.clients);
process.stdout.write(JSON.stringify(res));
