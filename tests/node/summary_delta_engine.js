'use strict';
// The incremental hand-over through the Node host path: BatchReplayEngine.markSummaryBaseline / summaryDelta /
// clearSummaryBaseline over one reference log.  Prints the delta against the marked baseline and, after clearing it,
// the delta again with the blob contents (base64); the Python test checks nulls, ids and bytes against hashlib.
// usage: node summary_delta_engine.js <replay.json.gz>
const fs = require('fs');
const zlib = require('zlib');
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const groups = JSON.parse(zlib.gunzipSync(fs.readFileSync(process.argv[2])).toString('utf8'));
const msgs = [].concat(...groups.map((g) => g.msgs));
const engine = new m.BatchReplayEngine(1, { snapshotV1: 1, maxSegments: 8192, heapEntries: 8192, textUnits: 1 << 18,
    propWords: 1 << 18, removerCells: 1 << 14, opsPerLaunch: 64 });
const c = engine.createClient();
if (groups[0].initialText) c.insertTextLocal(0, groups[0].initialText);
c.startOrUpdateCollaboration('A');
for (const msg of msgs) c.applyMsg(msg);
const last = msgs[msgs.length - 1];
const runtime = { deltaManager: { minimumSequenceNumber: last.minimumSequenceNumber,
    lastSequenceNumber: last.sequenceNumber } };
const s = c.summarize(runtime, undefined, undefined, undefined);
const show = (d) => ({ ids: d.ids, docFirst: d.docFirst,
    changed: d.changed.map((b) => (b === null ? null : b.toString('base64'))) });
const before = show(engine.summaryDelta(0, 1));
engine.markSummaryBaseline();
const marked = show(engine.summaryDelta(0, 1));
engine.clearSummaryBaseline();
const cleared = show(engine.summaryDelta());
process.stdout.write(JSON.stringify({ before, marked, cleared,
    blobs: Object.values(s.summary.tree).map((b) => Buffer.from(b.content, 'utf8').toString('base64')) }));
