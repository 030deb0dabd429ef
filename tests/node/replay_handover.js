'use strict';
// The hand-over that downloads only the blobs storage lacks, from the Node host (BatchReplayEngine.replayHandover ->
// the addon's replayHandover -> mtr_replay_handover): the reference replay logs (client.replay.spec.ts:17-71), every
// group but the last flushed as usual, the last applied, summarized and sorted against the blob-id cache in one call.
// The cache is seeded with the ids given in <held.json> (an array of hex ids).  Prints every blob's id, state, rep and
// bytes (base64, state 1 only), each document's first blob and whether the pipelined path ran, for the Python test to
// compare with the serial calls of the Python binding; then the tree ids, read without another summarize.
// mode "local": document 0 also queues a pending local insert before the call, so the batch holds a record the
// pipelined path refuses and the addon takes the serial calls (V1 summaries leave the unacked insert out).
// usage: node replay_handover.js <parts> <remote|local> <held.json> <replay.json.gz> [...]
const fs = require('fs');
const zlib = require('zlib');
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const parts = Number(process.argv[2]);
const mode = process.argv[3];
const held = JSON.parse(fs.readFileSync(process.argv[4], 'utf8'));
const files = process.argv.slice(5);
const all = files.map((f) => JSON.parse(zlib.gunzipSync(fs.readFileSync(f)).toString('utf8')));
const engine = new m.BatchReplayEngine(files.length, { snapshotV1: 1, maxSegments: 8192, heapEntries: 8192,
    textUnits: 1 << 18, propWords: 1 << 18, removerCells: 1 << 14, opsPerLaunch: 64 });
if (held.length) engine.blobCacheAdd(held);
const clients = all.map((groups) => {
    const c = engine.createClient();
    if (groups[0].initialText) c.insertTextLocal(0, groups[0].initialText);
    c.startOrUpdateCollaboration('A');
    return c;
});
const nGroups = Math.max(...all.map((g) => g.length));
let rec = null;
for (let gi = 0; gi < nGroups; gi++) {
    all.forEach((groups, d) => { if (gi < groups.length) for (const msg of groups[gi].msgs) clients[d].applyMsg(msg); });
    if (gi === nGroups - 1) {
        if (mode === 'local') clients[0].insertTextLocal(0, 'xyz');
        rec = engine.replayHandover(parts);
    } else {
        engine.flush();
    }
}
const blobs = rec.blobs.map((b) => ({ id: b.id, state: b.state, rep: b.rep,
    bytes: b.state === 1 ? b.bytes.toString('base64') : null }));
process.stdout.write(JSON.stringify({ pipelined: rec.pipelined, blobs, docFirst: Array.from(rec.docFirst),
    treeIds: engine.summaryTreeIds() }));
