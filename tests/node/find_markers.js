'use strict';
// BatchReplayEngine.findTiles, BatchReplayClient.findTile and BatchReplayClient.getMarkerFromId against a JS walk over
// getRangeSegments.  Two documents built from applyMsg: leaf j is appended with sequence number j + 1 (never merged:
// the minimum sequence number stays 0), a Tile marker with referenceTileLabels and markerId "m<j>" when j % 4 == 1,
// else three units of text; then client B removes marker leaf 5.  The walk knows a marker's labels by its sequence
// number (the rows carry the segment's seq, not its property values).  Prints what it compared for the Python test.
// usage: node find_markers.js
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const LABELS = [['Eop'], ['pg'], ['Eop', 'pg'], undefined];
const LEAVES = [70, 33];

function msg(clientId, contents, seq, ref) {
    return { clientId, sequenceNumber: seq, referenceSequenceNumber: ref, minimumSequenceNumber: 0, type: 'op', contents };
}
function rowsOf(engine, client, sequenceArgs) {
    return engine.getRangeSegments([{ client, sequenceArgs }])[0].map((r) => ({
        leaf: r.segment.leafIndex, start: r.segment._at.start, length: r.segment.cachedLength, seq: r.segment.seq,
        marker: r.segment.marker, props: r.segment.propertySet }));
}
function lengthOf(rows) {
    return rows.length ? rows[rows.length - 1].start + rows[rows.length - 1].length : 0;
}

function main() {
    const engine = new m.BatchReplayEngine(LEAVES.length, { snapshotV1: 1, maxSegments: 1024, heapEntries: 1024,
        textUnits: 1 << 12, propWords: 1 << 12, removerCells: 1 << 10, opsPerLaunch: 64 });
    const docs = LEAVES.map((leaves) => {
        const c = engine.createClient();
        c.startOrUpdateCollaboration('A');
        const labelsBySeq = new Map();
        let at = 0, removeAt = 0;
        for (let j = 0; j < leaves; j++) {
            let seg;
            if (j % 4 === 1) {
                const props = { markerId: 'm' + j };
                const labels = LABELS[(j >> 2) % 4];
                if (labels !== undefined) props.referenceTileLabels = labels;
                labelsBySeq.set(j + 1, labels || []);
                seg = { marker: { refType: 1 }, props };
                if (j === 5) removeAt = at;
            } else {
                seg = { text: 'abc' };
            }
            c.applyMsg(msg('W', { type: 0, pos1: at, seg }, j + 1, j));
            at += j % 4 === 1 ? 1 : 3;
        }
        c.applyMsg(msg('B', { type: 1, pos1: removeAt, pos2: removeAt + 1 }, leaves + 1, leaves));
        return { c, leaves, labelsBySeq };
    });
    const mismatches = [];
    const same = (a, b) => (a === undefined || b === undefined ? a === b
        : a.pos === b.pos && a.leaf === b.leaf && a.refType === b.refType && a.props === b.props && a.seq === b.seq);
    const expectTile = (d, rows, pos, label, preceding) => {
        const hits = rows.filter((r) => r.marker !== undefined && d.labelsBySeq.get(r.seq).includes(label) &&
            (preceding ? r.start <= pos : r.start >= pos));
        if (!hits.length) return undefined;
        const r = preceding ? hits[hits.length - 1] : hits[0];
        return { pos: r.start, leaf: r.leaf, refType: r.marker.refType, props: r.props === undefined ? -1 : r.props, seq: r.seq };
    };
    const queries = [], want = [];
    let found = 0, none = 0, singles = 0, ids = 0;
    docs.forEach((d) => {
        const views = [undefined, { referenceSequenceNumber: d.leaves, clientId: 'W' }, { referenceSequenceNumber: 20, clientId: 'B' }];
        for (const v of views) {
            const rows = rowsOf(engine, d.c, v);
            const len = lengthOf(rows);
            for (const pos of [-1, 0, 1, 3, 4, 5, 13, 14, 15, len >> 1, len - 1, len, len + 1, 0x7fffffff]) {
                for (const label of ['Eop', 'pg', 'nobody']) {
                    for (const preceding of [true, false, undefined]) {
                        queries.push({ client: d.c, pos, label, preceding,
                            refSeq: v && v.referenceSequenceNumber, clientId: v && v.clientId });
                        want.push(expectTile(d, rows, pos, label, preceding !== false));
                    }
                }
            }
        }
    });
    const got = engine.findTiles(queries);
    queries.forEach((q, i) => {
        if (!same(got[i], want[i])) mismatches.push(['findTiles', i, q.pos, q.label, q.preceding, q.refSeq, want[i], got[i]]);
        if (want[i] === undefined) none++; else found++;
    });
    docs.forEach((d, k) => {
        const rows = rowsOf(engine, d.c, undefined);
        for (const pos of [0, 14, lengthOf(rows) >> 1]) {
            for (const preceding of [true, false]) {
                const g = preceding ? d.c.findTile(pos, 'pg') : d.c.findTile(pos, 'pg', false);
                if (!same(g, expectTile(d, rows, pos, 'pg', preceding))) mismatches.push(['findTile', k, pos, preceding, g]);
                singles++;
            }
        }
        // getMarkerFromId: the marker "m<j>" is leaf j; its position is where the first row not below it starts
        // (the writer's view before the remove; B's own view at that refSeq already hides what B removed)
        const all = rowsOf(engine, d.c, { referenceSequenceNumber: d.leaves, clientId: 'W' });
        for (let j = 1; j < d.leaves; j += 4) {
            const row = rows.find((r) => r.leaf >= j);
            const src = all.find((r) => r.leaf === j);
            const exp = { pos: row === undefined ? lengthOf(rows) : row.start, leaf: j, refType: 1,
                props: src.props === undefined ? -1 : src.props, seq: j + 1 };
            const g = d.c.getMarkerFromId('m' + j);
            if (!same(g, exp)) mismatches.push(['getMarkerFromId', k, j, exp, g]);
            ids++;
        }
        for (const id of ['m0', 'nobody', '', 7]) {
            if (d.c.getMarkerFromId(id) !== undefined) mismatches.push(['getMarkerFromId', k, id]);
        }
    });
    const hidden = docs[0].c.getMarkerFromId('m5');  // removed, still in the tree: it sits where leaf 6 starts
    const empty = engine.findTiles([]).length;
    let refused = '';
    try { engine.findTiles([{ client: {}, pos: 0, label: 'pg' }]); } catch (e) { refused = e.message; }
    const lv = engine.interner.labelValues('referenceTileLabels', 'pg');
    const keysBefore = engine.interner.keys.size;
    const unknown = engine.interner.labelValues('no-such-key', 'pg');
    process.stdout.write(JSON.stringify({ docs: docs.length, queries: queries.length, found, none, singles, ids,
        mismatches: mismatches.slice(0, 5), hiddenLeaf: hidden && hidden.leaf, empty, refused, pgValues: lv[1].length,
        unknownKey: unknown[0] === undefined && unknown[1].length === 0 && engine.interner.keys.size === keysBefore }));
}
main();
