'use strict';
// Git tree ids through the Node host path: BatchReplayEngine.summaryTreeIds() and BatchReplayClient.summaryTreeId().
// Every id the engine gives is checked here against one computed in JS with crypto from the summarize() tree; the
// script prints what it compared and exits non-zero on a difference.
// usage: node tree_ids_engine.js replay <replay.json.gz>          one reference log, V1 format (no catch-up blob)
//        node tree_ids_engine.js catchup <docs.json> <chunk>      legacy format with a catch-up blob
const fs = require('fs');
const zlib = require('zlib');
const path = require('path');
const crypto = require('crypto');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const sha1 = (...parts) => { const h = crypto.createHash('sha1'); parts.forEach((p) => h.update(p)); return h.digest(); };
const blobId = (buf) => sha1('blob ' + buf.length + '\0', buf);
// entries: [{name, id: Buffer, tree?}] -> the git tree id (bytewise order, a subtree comparing as its name + '/')
function treeId(entries) {
    const key = (e) => Buffer.from(e.name + (e.tree ? '/' : ''), 'utf8');
    const sorted = entries.slice().sort((a, b) => Buffer.compare(key(a), key(b)));
    const body = Buffer.concat(sorted.map((e) => Buffer.concat([Buffer.from((e.tree ? '40000 ' : '100644 ') + e.name + '\0',
        'utf8'), e.id])));
    return sha1('tree ' + body.length + '\0', body).toString('hex');
}

const mode = process.argv[2];
let docs;
if (mode === 'replay') {
    const groups = JSON.parse(zlib.gunzipSync(fs.readFileSync(process.argv[3])).toString('utf8'));
    docs = [{ observer: 'A', initialText: groups[0].initialText, msgs: [].concat(...groups.map((g) => g.msgs)) }];
} else {
    docs = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
}
const chunk = mode === 'replay' ? 1 << 30 : Number(process.argv[4]);
const engine = new m.BatchReplayEngine(docs.length, { snapshotV1: mode === 'replay' ? 1 : 0, maxSegments: 8192,
    heapEntries: 8192, textUnits: 1 << 18, propWords: 1 << 18, removerCells: 1 << 14, opsPerLaunch: 64 });
const clients = docs.map((d) => {
    const c = engine.createClient();
    if (d.initialText) c.insertTextLocal(0, d.initialText);
    c.startOrUpdateCollaboration(d.observer);
    return c;
});
const n = Math.max(...docs.map((d) => d.msgs.length));
for (let k = 0; k < n; k += chunk) {
    docs.forEach((d, i) => { for (const msg of d.msgs.slice(k, k + chunk)) clients[i].applyMsg(msg); });
    clients[0].getText();
}
const result = docs.map((d, i) => {
    const last = d.msgs[d.msgs.length - 1];
    const runtime = { deltaManager: { minimumSequenceNumber: last.minimumSequenceNumber,
        lastSequenceNumber: last.sequenceNumber } };
    const s = clients[i].summarize(runtime, undefined, undefined, undefined);
    const entries = Object.entries(s.summary.tree).map(([name, b]) => ({ name, id: blobId(Buffer.from(b.content, 'utf8')) }));
    const want = treeId(entries);
    const got = clients[i].summaryTreeId();
    if (got !== want) throw new Error(`document ${i}: summaryTreeId ${got}, crypto ${want}`);
    return { doc: i, names: entries.map((e) => e.name), id: got, entries };
});
// the range call: the engine's blobs alone, then with each document's host blobs passed as extras
const engineNames = (r) => r.entries.filter((e) => /^(header|body|body_\d+)$/.test(e.name));
const plain = engine.summaryTreeIds(0, docs.length);
const extras = result.map((r) => r.entries.filter((e) => !engineNames(r).includes(e))
    .map((e) => ({ name: e.name, id: e.id.toString('hex') })));
const full = engine.summaryTreeIds(0, docs.length, extras);
result.forEach((r, i) => {
    if (plain[i] !== treeId(engineNames(r))) throw new Error(`document ${i}: summaryTreeIds without extras differs`);
    if (full[i] !== r.id) throw new Error(`document ${i}: summaryTreeIds with extras differs`);
});
if (engine.summaryTreeIds(0, 0).length !== 0) throw new Error('an empty range should give no ids');
// a subtree entry and a sub-range
const sub = engine.summaryTreeIds(docs.length - 1, docs.length, [[{ name: 'intervals', id: result[0].id, tree: true }]])[0];
const lastDoc = result[docs.length - 1];
if (sub !== treeId(engineNames(lastDoc).concat([{ name: 'intervals', id: Buffer.from(result[0].id, 'hex'), tree: true }]))) {
    throw new Error('a subtree extra differs');
}
let refused = false;
try { engine.summaryTreeIds(0, 1, [[{ name: 'header', id: result[0].id }]]); } catch (e) { refused = /document 0/.test(String(e)); }
if (!refused) throw new Error('an extra named header should be refused, naming the document');
const nativeKeys = Object.keys(require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'mtr_napi.node')));
process.stdout.write(JSON.stringify({ docs: result.map((r) => ({ doc: r.doc, names: r.names, id: r.id })), plain,
    enumerable: nativeKeys.includes('summaryTreeIds') }));
