'use strict';
// BatchReplayEngine.getRangeSegments / getTextRanges and BatchReplayClient.getText(start, end) against the walk of
// BatchReplayClient.getContainingSegment that defines them: p = start; the segment holding p; p = its start + its
// length; until no segment covers p or p >= end.  Reference replay logs stopped mid-collaboration, one mixed batch of
// ranges interleaved across the documents, with and without sequenceArgs.  Prints what it compared for the Python test.
// usage: node range_queries.js <groups to apply> <replay.json.gz> [...]
const fs = require('fs');
const zlib = require('zlib');
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

function shown(r) {
    return JSON.stringify([r, r.segment === undefined ? null : r.segment._at]);
}

// the walk: [{result with its text clipped to the range}], and the range's text
function walk(q, placeholder) {
    const start = q.start === undefined ? 0 : q.start, end = q.end === undefined ? 0x7fffffff : q.end;
    const out = [];
    let text = '';
    for (let p = start; p < end;) {
        const r = q.client.getContainingSegment(p, q.sequenceArgs);
        if (r.segment === undefined) break;
        const s0 = r.segment._at.start, len = r.segment.cachedLength;
        if (r.segment.marker === undefined) {
            r.segment.text = r.segment.text.slice(Math.max(start - s0, 0), Math.min(end - s0, len));
            text += r.segment.text;
        } else {
            text += placeholder || '';
        }
        out.push(r);
        p = s0 + len;
    }
    return { segments: out, text };
}

function main() {
    const nGroups = Number(process.argv[2]);
    const files = process.argv.slice(3);
    const all = files.map((f) => JSON.parse(zlib.gunzipSync(fs.readFileSync(f)).toString('utf8')));
    const engine = new m.BatchReplayEngine(files.length, { snapshotV1: 1, maxSegments: 8192, heapEntries: 8192,
        textUnits: 1 << 18, propWords: 1 << 18, removerCells: 1 << 14, opsPerLaunch: 64 });
    const clients = [];
    const perDoc = all.map((groups) => {
        const c = engine.createClient();
        clients.push(c);
        if (groups[0].initialText) c.insertTextLocal(0, groups[0].initialText);
        c.startOrUpdateCollaboration('A');
        const msgs = [];
        for (const g of groups.slice(0, nGroups)) for (const msg of g.msgs) { c.applyMsg(msg); msgs.push(msg); }
        const cur = msgs[msgs.length - 1].sequenceNumber;
        const writers = [...new Set(msgs.map((x) => x.clientId))].filter((x) => x !== null && x !== undefined);
        const len = c.getLength();
        const qs = [{ client: c }, { client: c, start: 1, end: len - 1 }, { client: c, start: len >> 1, end: len >> 1 },
            { client: c, start: len >> 1, end: (len >> 1) + 1 }, { client: c, start: len, end: len + 4 },
            { client: c, start: len - 2 }, { client: c, end: 3 }];
        writers.forEach((w, k) => {
            for (const back of [0, 5]) {
                const sequenceArgs = { referenceSequenceNumber: Math.max(0, cur - back), clientId: w };
                qs.push({ client: c, start: (len >> 2) + k, end: (len >> 1) + 2 * k, sequenceArgs });
                qs.push({ client: c, start: k, sequenceArgs });
            }
        });
        return qs;
    });
    const queries = [];
    for (let k = 0; k < Math.max(...perDoc.map((q) => q.length)); k++) {
        for (const qs of perDoc) if (k < qs.length) queries.push(qs[k]);
    }
    const mismatches = [];
    let segments = 0, markers = 0, clipped = 0;
    for (const placeholder of [undefined, '*']) {
        const batched = engine.getRangeSegments(queries, placeholder);
        const texts = engine.getTextRanges(queries, placeholder);
        queries.forEach((q, i) => {
            const want = walk(q, placeholder);
            const a = JSON.stringify(want.segments.map(shown)), b = JSON.stringify(batched[i].map(shown));
            if (a !== b) mismatches.push(['segments', i, a.slice(0, 300), b.slice(0, 300)]);
            if (texts[i] !== want.text) mismatches.push(['text', i, want.text.slice(0, 80), texts[i].slice(0, 80)]);
            segments += want.segments.length;
            for (const r of want.segments) {
                if (r.segment.marker !== undefined) markers++;
                else if (r.segment.text.length < r.segment.cachedLength) clipped++;
            }
        });
    }
    // getText(start, end) on a client; without arguments it is the whole local view, as before
    let getText = 0;
    clients.forEach((c, d) => {
        const len = c.getLength(), whole = c.getText();
        if (engine.getTextRanges([{ client: c }])[0] !== whole) mismatches.push(['whole', d]);
        for (const [a, b] of [[0, len], [1, len - 1], [len >> 1, undefined], [undefined, 4], [len, len + 1]]) {
            const want = walk({ client: c, start: a, end: b }).text;
            if (c.getText(a, b) !== want) mismatches.push(['getText', d, a, b]);
            getText++;
        }
    });
    const none = [engine.getRangeSegments([]).length, engine.getTextRanges([]).length];
    let refused = '';
    try {
        engine.getRangeSegments([{ client: {}, start: 0, end: 1 }]);
    } catch (e) { refused = e.message; }
    let bad = '';
    try {
        engine.getTextRanges([{ client: clients[0], start: 5, end: 4 }]);
    } catch (e) { bad = e.message; }
    process.stdout.write(JSON.stringify({ docs: files.length, queries: queries.length, segments, markers, clipped, getText,
        mismatches: mismatches.slice(0, 5), empty: none, refused, bad }));
}
main();
