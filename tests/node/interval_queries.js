'use strict';
/*
 * The Node host's device interval queries (tests/test_node_interval_queries.py, -m gpu): Collection.
 * findOverlappingIntervals / previousInterval / nextInterval of fluidframework_amd/node/intervals.js over
 * mtr_query_intervals, on one interval-farm document, against the answers the Python host gave for the same probes.
 * argv[2]: a JSON file {init, msgs, labels: {label: {overlaps: [[a, b, [ids]]], ends: [[pos, prev, next]]}}}, prev /
 * next an id, null (no interval) or "refused".  Prints {compared, refused, overlaps, mismatches, records}.
 */
const fs = require('fs');
const path = require('path');
const { BatchReplayEngine } = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const input = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const engine = new BatchReplayEngine(4);
const client = engine.createClient();
client.insertTextLocal(0, input.init);
client.startOrUpdateCollaboration('observer', 0, 0);
for (const m of input.msgs) client.applyMsg(m, false);

const out = { compared: 0, refused: 0, overlaps: 0, mismatches: [], records: 0 };
const ask = (fn) => {
    try {
        const iv = fn();
        return iv === undefined ? null : iv.id();
    } catch (e) {
        if (e.name !== 'UnsupportedError') throw e;
        return 'refused';
    }
};
for (const label of Object.keys(input.labels)) {
    const c = client.getIntervalCollection(label).device;
    const want = input.labels[label];
    client.refKeys();  // (everything pending is applied: the queries below must queue nothing)
    const before = client.log.ops.length;
    const got = c.findOverlappingIntervalsMany(want.overlaps.map(([a, b]) => [a, b]));
    want.overlaps.forEach(([a, b, ids], k) => {
        out.overlaps++;
        const g = got[k].map((iv) => iv.id());
        if (JSON.stringify(g) !== JSON.stringify(ids)) out.mismatches.push([label, 'overlap', a, b, g, ids]);
    });
    for (const [pos, prev, next] of want.ends) {
        for (const [name, w] of [['previousInterval', prev], ['nextInterval', next]]) {
            const g = ask(() => c[name](pos));
            if (g === 'refused') out.refused++; else out.compared++;
            if (g !== w) out.mismatches.push([label, name, pos, g, w]);
        }
    }
    out.records += client.log.ops.length - before;
}
console.log(JSON.stringify(out));
