'use strict';
// The blob-id cache through the Node host path: BatchReplayEngine.blobCacheAdd / blobCacheAddSummary / blobCacheHas /
// blobCacheSize / blobCacheClear / summaryNovel over a fleet of documents that mostly replay one reference log.
// Prints summaryNovel without a cache, after blobCacheAddSummary, and against a cache of the ids the test passes in,
// with every blob's contents (base64); the Python test checks them against gitid.summary_novel.
// usage: node blob_cache_engine.js <template replay.json.gz> <other replay.json.gz> <docs> <pick>
//   document d replays the other log when d % 7 == 3, else the template; after the first two rounds the cache is
//   cleared and holds every distinct id whose rank in sorted order is a multiple of <pick>
const fs = require('fs');
const zlib = require('zlib');
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const load = (p) => JSON.parse(zlib.gunzipSync(fs.readFileSync(p)).toString('utf8'));
const logs = [load(process.argv[2]), load(process.argv[3])];
const docs = Number(process.argv[4]);
const pick = Number(process.argv[5]);
const engine = new m.BatchReplayEngine(docs, { snapshotV1: 1, chunkSize: 8, maxSegments: 4096, heapEntries: 4096,
    textUnits: 1 << 16, propWords: 1 << 14, removerCells: 1 << 12, opsPerLaunch: 64 });
const clients = [];
for (let d = 0; d < docs; d++) {
    const groups = logs[d % 7 === 3 ? 1 : 0];
    const c = engine.createClient();
    if (groups[0].initialText) c.insertTextLocal(0, groups[0].initialText);
    c.startOrUpdateCollaboration('A');
    for (const g of groups) for (const msg of g.msgs) c.applyMsg(msg);
    clients.push([c, groups[groups.length - 1].msgs]);
}
const blobs = clients.map(([c, msgs]) => {
    const last = msgs[msgs.length - 1];
    const s = c.summarize({ deltaManager: { minimumSequenceNumber: last.minimumSequenceNumber,
        lastSequenceNumber: last.sequenceNumber } }, undefined, undefined, undefined);
    return Object.values(s.summary.tree).map((b) => Buffer.from(b.content, 'utf8').toString('base64'));
});
const show = (rows) => rows.map((r) => ({ id: r.id, state: r.state, rep: r.rep,
    bytes: r.bytes === undefined ? null : r.bytes.toString('base64') }));
const sizes = [engine.blobCacheSize()];
const none = show(engine.summaryNovel());
engine.blobCacheAddSummary();
sizes.push(engine.blobCacheSize());
const acknowledged = show(engine.summaryNovel(0, docs));
const distinct = Array.from(new Set(none.map((r) => r.id))).sort();
const hasAll = engine.blobCacheHas(distinct);
engine.blobCacheClear();
sizes.push(engine.blobCacheSize());
const cache = distinct.filter((_, k) => k % pick === 0);
engine.blobCacheAdd(cache);
engine.blobCacheAdd(Buffer.from(cache.join(''), 'hex'));  // (the same ids as a Buffer: absorbed)
sizes.push(engine.blobCacheSize());
const has = engine.blobCacheHas(distinct);
const partial = show(engine.summaryNovel());
const middle = show(engine.summaryNovel(2, 9));
process.stdout.write(JSON.stringify({ blobs, none, acknowledged, partial, middle, cache, distinct, has, hasAll, sizes }));
