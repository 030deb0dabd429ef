'use strict';
// The blob-id cache's life cycle through the Node host path: BatchReplayEngine.blobCacheGeneration / blobCacheAges /
// blobCacheTrim / blobCacheTrimTo / blobCacheExport / blobCacheImport.  Runs a fixed sequence of calls over the ids
// the test passes in and prints what the cache shows after every step; the Python test runs gitid.BlobCacheModel
// through the same sequence and compares.
// usage: node blob_cache_trim_engine.js <ids.json: an array of 40-digit hex ids, even and odd ones alternating>
const fs = require('fs');
const path = require('path');
const m = require(path.join(__dirname, '..', '..', 'fluidframework_amd', 'node', 'index.js'));

const ids = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const caps = { snapshotV1: 1, chunkSize: 8, maxSegments: 4096, heapEntries: 4096, textUnits: 1 << 16,
    propWords: 1 << 14, removerCells: 1 << 12, opsPerLaunch: 64 };
const even = ids.filter((_, k) => k % 2 === 0);
const odd = ids.filter((_, k) => k % 2 === 1).reverse();
const hexes = (buf) => Array.from({ length: buf.length / 20 }, (_, k) => buf.toString('hex', 20 * k, 20 * k + 20));
const steps = [];
const snap = (name, engine, extra) => {
    const e = engine.blobCacheExport();
    steps.push(Object.assign({ name, size: engine.blobCacheSize(), generation: engine.blobCacheGeneration(),
        ids: hexes(e.ids), ages: e.ages, ages4: engine.blobCacheAges(4), has: engine.blobCacheHas(ids) }, extra || {}));
};

// trim rebuilds the probe chains: every other id of each chain goes
const a = new m.BatchReplayEngine(1, caps);
snap('empty', a);
a.blobCacheAdd(even);
a.blobCacheImport([ids[0]], [1]);  // generation 1; the entry keeps stamp 0
a.blobCacheAdd(Buffer.from(odd.join(''), 'hex'));
snap('two generations', a);
snap('trim', a, { removed: a.blobCacheTrim(1) });
a.blobCacheAdd([ids[4]]);
snap('a removed id again', a);
// export and import across engines
a.blobCacheImport(even.slice(0, 50), Array.from({ length: 50 }, (_, k) => 2 + (k % 3)));
snap('older entries', a);
const b = new m.BatchReplayEngine(1, caps);
const exported = a.blobCacheExport();
b.blobCacheImport(exported.ids, exported.ages);
snap('imported', b);
b.blobCacheImport([], []);
snap('imported nothing', b);
snap('trim to 320', b, { removed: b.blobCacheTrimTo(320) });
snap('trim to 0', b, { removed: b.blobCacheTrimTo(0) });
snap('the first engine', a);
let refused = null;
try { a.blobCacheAges(1025); } catch (err) { refused = String(err.message); }
process.stdout.write(JSON.stringify({ steps, refused }));
