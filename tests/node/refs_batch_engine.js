'use strict';
// BatchReplayEngine.getRefsBatch against the per-document calls (getRefPositions, getRefStates, getRefKeys): an empty
// document, one with text and no reference, one with 65 references (a second 64-reference block) and one whose
// references sit on removed text.  Prints what it compared for the Python test.
const path = require('path');
const dir = path.join(__dirname, '..', '..', 'fluidframework_amd', 'node');
const m = require(path.join(dir, 'index.js'));
const native = require(path.join(dir, 'mtr_napi.node'));

const SlideOnRemove = 0x40, Simple = 0;

function main() {
    const engine = new m.BatchReplayEngine(4, { snapshotV1: 1, maxSegments: 1024, heapEntries: 1024, textUnits: 1 << 14,
        propWords: 1 << 10, removerCells: 1 << 10, opsPerLaunch: 64, refSlots: 256 });
    const clients = [0, 1, 2, 3].map(() => engine.createClient());
    clients[1].insertTextLocal(0, 'no references here');
    for (let i = 0; i < 13; i++) clients[2].insertTextLocal(0, 'abcde');
    for (let r = 0; r < 65; r++) clients[2].createPositionReference(r, SlideOnRemove);
    clients[3].insertTextLocal(0, '0123456789');
    clients[3].insertTextLocal(5, 'ABCD');
    clients[3].startOrUpdateCollaboration('A');
    for (const pos of [0, 4, 6, 13]) clients[3].createPositionReference(pos, pos & 1 ? Simple : SlideOnRemove);
    clients[3].removeRangeLocal(4, 8);
    engine.flush();

    const single = {
        1: (c) => native.getRefPositions(engine.h, c.doc),
        2: (c) => native.getRefStates(engine.h, c.doc),
        4: (c) => c.refKeys(),
    };
    const order = [2, 0, 3, 1, 2];  // scrambled, one client twice
    const mismatches = [];
    const counts = {};
    for (const mode of [1, 2, 4]) {
        const got = engine.getRefsBatch(order.map((k) => clients[k]), mode);
        let at = 0;
        order.forEach((k, i) => {
            const want = Array.from(single[mode](clients[k]));
            if (got.docFirst[i] !== at) mismatches.push([mode, i, 'docFirst', got.docFirst[i], at]);
            const mine = Array.from(got.words.subarray(mode * at, mode * at + want.length));
            if (JSON.stringify(mine) !== JSON.stringify(want)) mismatches.push([mode, i, mine, want]);
            at += want.length / mode;
        });
        if (got.docFirst[order.length] !== at || got.words.length !== mode * at) mismatches.push([mode, 'total', at]);
        counts[mode] = at;
    }
    const none = engine.getRefsBatch([clients[0], clients[1]], 2);
    let refused = '';
    try {
        engine.getRefsBatch([{}], 2);
    } catch (e) { refused = e.message; }
    let badMode = '';
    try {
        engine.getRefsBatch([clients[2]], 3);
    } catch (e) { badMode = e.message; }
    process.stdout.write(JSON.stringify({ counts, mismatches: mismatches.slice(0, 5), emptyTotal: none.docFirst[2],
        emptyWords: none.words.length, refused, badMode, enumerable: Object.keys(native).includes('getRefsBatch'),
        positions65: Array.from(native.getRefPositions(engine.h, clients[2].doc)).length }));
}
main();
