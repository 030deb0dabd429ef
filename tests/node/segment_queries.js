'use strict';
// BatchReplayEngine.getContainingSegments against a loop of BatchReplayClient.getContainingSegment: reference replay
// logs stopped mid-collaboration, then one mixed batch -- queries interleaved across the documents, with and without
// sequenceArgs, every writer's view, positions from -1 to one past the end.  Prints what it compared for the Python
// test.
// usage: node segment_queries.js <groups to apply> <replay.json.gz> [...]
const fs = require('fs');
const zlib = require('zlib');
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

// a result with the hidden anchor createLocalReferencePosition reads (non-enumerable: JSON alone would drop it)
function shown(r) {
    return JSON.stringify([r, r.segment === undefined ? null : r.segment._at]);
}

function main() {
    const nGroups = Number(process.argv[2]);
    const files = process.argv.slice(3);
    const all = files.map((f) => JSON.parse(zlib.gunzipSync(fs.readFileSync(f)).toString('utf8')));
    const engine = new m.BatchReplayEngine(files.length, { snapshotV1: 1, maxSegments: 8192, heapEntries: 8192,
        textUnits: 1 << 18, propWords: 1 << 18, removerCells: 1 << 14, opsPerLaunch: 64 });
    const perDoc = all.map((groups) => {
        const c = engine.createClient();
        if (groups[0].initialText) c.insertTextLocal(0, groups[0].initialText);
        c.startOrUpdateCollaboration('A');
        const msgs = [];
        for (const g of groups.slice(0, nGroups)) for (const msg of g.msgs) { c.applyMsg(msg); msgs.push(msg); }
        const cur = msgs[msgs.length - 1].sequenceNumber;
        const writers = [...new Set(msgs.map((x) => x.clientId))].filter((x) => x !== null && x !== undefined);
        const len = c.getLength();
        const qs = [];
        for (const pos of [-1, 0, 1, len >> 1, len - 1, len, len + 1]) qs.push({ client: c, pos });
        writers.forEach((w, k) => {
            for (const back of [0, 3, 9]) {
                const sequenceArgs = { referenceSequenceNumber: Math.max(0, cur - back), clientId: w };
                for (const pos of [0, (len >> 2) + k, (len >> 1) + k, len - 1 - k]) qs.push({ client: c, pos, sequenceArgs });
            }
        });
        return qs;
    });
    const queries = [];
    for (let k = 0; k < Math.max(...perDoc.map((q) => q.length)); k++) {
        for (const qs of perDoc) if (k < qs.length) queries.push(qs[k]);
    }
    const batched = engine.getContainingSegments(queries);
    let segments = 0, texts = 0, markers = 0;
    const mismatches = [];
    queries.forEach((q, i) => {
        const one = q.client.getContainingSegment(q.pos, q.sequenceArgs);
        if (shown(one) !== shown(batched[i])) mismatches.push([i, shown(one), shown(batched[i])]);
        if (one.segment !== undefined) {
            segments++;
            if (one.segment.text !== undefined && one.segment.text.length === one.segment.cachedLength) texts++;
            if (one.segment.marker !== undefined) markers++;
        }
    });
    const none = engine.getContainingSegments([]);
    let refused = '';
    try {
        engine.getContainingSegments([{ client: {}, pos: 0 }]);
    } catch (e) { refused = e.message; }
    process.stdout.write(JSON.stringify({ docs: files.length, queries: queries.length, results: batched.length, segments,
        texts, markers, mismatches: mismatches.slice(0, 5), empty: none.length, refused }));
}
main();
