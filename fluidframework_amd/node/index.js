'use strict';
/*
 * Node host side of the MI355X merge-tree replay engine: the observer subset of
 * @fluidframework/merge-tree's Client (packages/dds/merge-tree/src/client.ts:98) over the N-API
 * addon (mtr_napi.cc) and the C ABI (include/mtr.h).
 *
 *   reference                                          | here
 *   ---------------------------------------------------+--------------------------------------------
 *   new Client(specToSegment, logger, options)         | engine.createClient()   (one engine = many docs)
 *   client.startOrUpdateCollaboration(id, min, cur)    | same name              (client.ts:1133)
 *   client.applyMsg(msg)                               | same name              (client.ts:858)
 *   client.updateSeqNumbers(min, seq)                  | same name              (client.ts:877)
 *   client.insertTextLocal / removeRangeLocal /        | same names, before collaboration only
 *     annotateRangeLocal (non-collaborating edits)     |   (client.ts:237-285)
 *   client.summarize(runtime, handle, ser, catchUp)    | same name              (client.ts:966)
 *   client.getText() / getLength() / getCurrentSeq()   | same names
 *
 * Messages are packed on the JS thread exactly as the reference reads them (short client ids in
 * first-seen order, GROUP ops flattened, JSON.stringify / Object.keys for property values and key
 * order) and applied on the GPU in batches: applyMsg only queues, and the queue is flushed -- for
 * every document of the engine at once -- before anything is read back.  Results are identical to
 * applying each message synchronously because nothing observable happens in between.
 * Written for Node >= 12 (no optional chaining).
 */
const path = require('path');
const { IntervalCollections, IntervalUnsupported, refKey, cmpKey } = require('./intervals.js');

let addon = null;
function native() {
    if (addon === null) addon = require(path.join(__dirname, 'mtr_napi.node'));
    return addon;
}

// include/mtr_types.h
const OP = { INSERT: 0, REMOVE: 1, ANNOTATE: 2, SEQ: 3, LOCAL_INSERT: 8, LOCAL_REMOVE: 9, LOCAL_ANNOTATE: 10,
    START_COLLAB: 12, LOAD: 13, SETCELL: 14, RELPOS: 15, ACK: 17, ROLLBACK: 18, REGENERATE: 19, REF_CREATE: 20, REF_REMOVE: 21,
    REF_ACK: 24, REBASE_POS: 25, LSEQ: 26 };
const REF = { SLIDE: 1, LOCALVIEW: 2, LSEQ: 4, SLOT: 8 };  // MTR_OP_REF_CREATE payload2
const DELTA_REBASE = 80;
const POS_FROM_VIEW = 0, POS_FROM_LEAF = 1;  // include/mtr.h MTR_POS_FROM_VIEW / _FROM_LEAF
const MK_PRECEDING = 0, MK_FOLLOWING = 1, MK_BY_ID = 2, MK_FOUND = 1;  // include/mtr.h MTR_MK_*
const TILE_LABELS_KEY = 'referenceTileLabels';
const DetachedReferencePosition = -1;   // referencePositions.ts:103
const DELTA_REGEN = 64, DELTA_REGEN_X = 72;
const REL = { BEFORE: 1, OFFSET: 2 };
const COMB = { NONE: 0, REWRITE: 1, INCR: 2, CONSENSUS: 3, KEEP: 4 };
const VEQ = { NEVER: 0x80000000, FALSY: 0x40000000, INCR_STR: 0x20000000, CONS_MUT: 0x10000000 };
const F = { LAST: 1, MARKER: 2, PROPS: 4, NOREF: 8, APPEND: 16, COLS: 32, DELTA: 64, REL: 128 };
const CLIENT_NONCOLLAB = 0xFFFE;  // include/mtr_types.h MTR_CLIENT_NONCOLLAB
const NULL_VALUE = 0xFFFFFFFF;
const MAX_CLIENTS = 253;  // include/mtr_types.h MTR_MAX_CLIENTS: short ids per engine document
const NOT_INDEX = 0xFFFFFFFF;
const STATUS = { OK: 0, INSERT_FAILED: 1, BAD_OP: 2, CAPACITY: 3, UNSUPPORTED: 4, ASSERT: 0x1000 };
// protocol-definitions SummaryType
const SummaryType = { Tree: 1, Blob: 2 };

class UnsupportedError extends Error {
    constructor(msg) {
        super(msg);
        this.name = 'UnsupportedError';
        this.fallback = true;  // the document must stay on the TypeScript Client
    }
}

function arrayIndex(key) {
    if (/^(0|[1-9][0-9]*)$/.test(key)) {
        const v = Number(key);
        if (v < 4294967295) return v;
    }
    return null;
}

/*
 * matchProperties (properties.ts:71-105) compares values by strict equality and recurses into any
 * `typeof === "object"` value through `for...in`, so arrays and index-keyed objects compare equal.
 * That is an equivalence -- and interning equivalence classes is exact -- for values without
 * nested nulls and empty containers; documents with such values stay on the TypeScript Client.
 */
let nanCounter = 0;
function eqKey(v) {
    if (typeof v === 'boolean') return v ? 'true' : 'false';
    if (typeof v === 'number') return Number.isNaN(v) ? 'NaN#' + (nanCounter++) : 'n' + String(v === 0 ? 0 : v);
    if (typeof v === 'string') return 's' + JSON.stringify(v);
    return '{' + Object.keys(v).sort().map((k) => JSON.stringify(k) + ':' + eqKey(v[k])).join(',') + '}';
}
function plainValue(v, nested) {
    if (v === null) return !nested;  // a top-level null deletes the key
    if (typeof v !== 'object') return true;
    const keys = Object.keys(v);
    if (keys.length === 0) return false;
    return keys.every((k) => plainValue(v[k], true));
}

const utf8 = (s) => Buffer.from(s, 'utf8');

// MTR_VEQ_* bits of a JSON value (include/mtr_types.h)
function valueFlags(v) {
    let f = 0;
    if (!v) f |= VEQ.FALSY;
    if (typeof v === 'string' || (v !== null && typeof v === 'object')) f |= VEQ.INCR_STR;  // v + undefined concatenates
    if (v !== null && typeof v === 'object' && !Array.isArray(v) && v.seq === -1) f |= VEQ.CONS_MUT;
    return f >>> 0;
}

const NAN = { nan: true };  // combine results that are not JSON values
class Never { constructor(json) { this.json = json; } }

// combine(co, undefined, undefined, seq) (properties.ts:24-69) for a key the segment lacks
function combineAbsent(co, seq) {
    const cur = co.defaultValue;
    if (co.name === 'incr') {
        if (cur === undefined || cur === null || typeof cur === 'number' || typeof cur === 'boolean') return NAN;
        if (typeof cur !== 'string') throw new UnsupportedError('incr of a non-primitive default value');
        let r = cur + 'undefined';
        const mv = co.minValue;
        if (mv) {
            if (typeof mv === 'string') { if (r < mv) r = mv; } else if (typeof mv !== 'number') {
                throw new UnsupportedError('incr minValue comparison');
            }
        }
        return r;
    }
    if (co.name === 'consensus') {
        if (cur === undefined) return new Never('{"seq":' + seq + '}');  // {value: undefined, seq}
        if (cur === null) throw new UnsupportedError('consensus on a null default (TypeError in the reference)');
        if (typeof cur === 'object' && !Array.isArray(cur) && cur.seq === -1) return Object.assign({}, cur, { seq });
        return cur;
    }
    if (cur === undefined) throw new UnsupportedError('combiningOp without a default leaves an explicit undefined property');
    return cur;
}

/** Global key / value / prop-op tables (ids stable across batches). */
class Interner {
    constructor() {
        this.keys = new Map(); this.keyBytes = []; this.keyIndex = [];
        this.vals = new Map(); this.valBytes = []; this.valEq = []; this.eqIds = new Map();
        this.propops = []; this.never = new Map();
        // labelValues' cache: the array values among the first _labelSeen entries of vals, [value id, its string members]
        this._labelArrays = []; this._labelSeen = 0;
    }
    /**
     * [key id, [value ids]] for a label search under property `key`: the ids, ascending, of the values whose JSON text
     * is an array holding the string `label` -- what mtr_find_markers' label table takes.  [undefined, []] when the key
     * was never interned: no marker can match, and no key is created.  The array values seen so far are kept; the
     * value table's growth since the last call is read on the next.
     */
    labelValues(key, label) {
        if (this.vals.size > this._labelSeen) {
            let k = 0;
            for (const [s, i] of this.vals) {  // (a Map iterates in insertion order: the new entries are the last)
                if (k++ < this._labelSeen || s[0] !== '[') continue;
                const v = JSON.parse(s);
                if (Array.isArray(v)) this._labelArrays.push([i, new Set(v.filter((x) => typeof x === 'string'))]);
            }
            this._labelSeen = this.vals.size;
        }
        const id = this.keys.get(key);
        if (id === undefined) return [undefined, []];
        return [id, this._labelArrays.filter(([, members]) => members.has(label)).map(([i]) => i)];
    }
    _addValue(s, eq) {
        const i = this.valBytes.length;
        this.valBytes.push(utf8(s));
        this.valEq.push(eq >>> 0);
        return i;
    }
    neverValue(s) {  // matchProperties never matches it, not even with itself
        let i = this.never.get(s);
        if (i === undefined) {
            const e = this.eqIds.size;
            this.eqIds.set('never#' + e, e);
            i = this._addValue(s, (e | VEQ.NEVER) >>> 0);
            this.never.set(s, i);
        }
        return i;
    }
    nan() { return this.neverValue('null'); }
    _valueOrNull(r) {
        if (r === NAN) return this.nan();
        if (r instanceof Never) return this.neverValue(r.json);
        if (r === null) return NULL_VALUE;
        return this.value(r);
    }
    // a remote annotate with combiningOp co -> [propop, payload2] (include/mtr_types.h MTR_COMB_*)
    combining(props, co, seq) {
        if (props === null || typeof props !== 'object' || Array.isArray(props)) throw new UnsupportedError('annotate props');
        if (!co) return [this.propop(props), COMB.NONE];
        if (typeof co !== 'object' || Array.isArray(co)) throw new UnsupportedError('combiningOp');
        if (co.name === 'rewrite') return [this.propop(props), COMB.REWRITE];
        const mode = co.name === 'incr' ? COMB.INCR : (co.name === 'consensus' ? COMB.CONSENSUS : COMB.KEEP);
        const absent = this._valueOrNull(combineAbsent(co, seq));
        this.propops.push(Object.keys(props).map((k) => [this.key(k), absent]));
        return [this.propops.length - 1, mode === COMB.INCR ? (mode | (this.nan() << 3)) >>> 0 : mode];
    }
    key(k) {
        let i = this.keys.get(k);
        if (i === undefined) {
            i = this.keyBytes.length;
            this.keys.set(k, i);
            this.keyBytes.push(utf8(JSON.stringify(k).slice(1, -1)));
            const ix = arrayIndex(k);
            this.keyIndex.push(ix === null ? NOT_INDEX : ix);
        }
        return i;
    }
    value(v) {
        if (v === null) return NULL_VALUE;
        if (!plainValue(v, false)) throw new UnsupportedError('property value with nested null or empty container');
        const s = JSON.stringify(v);
        let i = this.vals.get(s);
        if (i === undefined) {
            const ek = eqKey(v);
            let e = this.eqIds.get(ek);
            if (e === undefined) { e = this.eqIds.size; this.eqIds.set(ek, e); }
            i = this._addValue(s, (e | valueFlags(v)) >>> 0);
            this.vals.set(s, i);
        }
        return i;
    }
    propop(props) {  // Object.keys order = JS own-key order
        this.propops.push(Object.keys(props).map((k) => [this.key(k), this.value(props[k])]));
        return this.propops.length - 1;
    }
}

/** Per-document host state: client registry plus the queued ops/text of the next batch. */
class DocLog {
    constructor() {
        this.observerId = undefined; this.clients = []; this.clientIx = new Map();
        this.ops = []; this.text = []; this.collaborating = false;
        // MergeTree.idToSegment (mergeTree.ts:549,668) as the host sees it: id key -> marker ordinal
        this.nMarkers = 0; this.markerIds = new Map(); this.markerDup = new Set(); this.markerIdAnnotated = false;
        this.nRefs = 0;  // reference ids handed out (MTR_OP_REF_CREATE ids; high-water mark)
        this.freeRefs = [];  // ids released for reuse (MTR_REF_SLOT), a stack
        this.currentSeq = 0;  // collabWindow.currentSeq as the host sees it (interval ops do not move it)
        this.intervals = undefined;  // ./intervals.js IntervalCollections, when used
    }
    _intervals(fn) {  // an interval path this host does not restate is an UnsupportedError (the document falls back)
        try {
            return fn();
        } catch (e) {
            if (e instanceof IntervalUnsupported) throw new UnsupportedError(e.message);
            throw e;
        }
    }
    static _idKey(v) {  // SameValueZero keys; objects only match themselves (never from JSON)
        if (typeof v === 'boolean') return 'b' + v;
        if (typeof v === 'number') return 'n' + String(v === 0 ? 0 : v);
        if (typeof v === 'string') return 's' + v;
        return null;
    }
    _mapMarker(props) {  // Marker.getId truthy -> mapIdToSegment: ordinal + 1 (0 = no id)
        if (!props || typeof props !== 'object' || !props.markerId) return 0;
        const k = DocLog._idKey(props.markerId);
        const o = this.nMarkers++;
        if (k !== null) {
            if (this.markerIds.has(k)) this.markerDup.add(k);
            this.markerIds.set(k, o);
        }
        return o + 1;
    }
    _relpos(rp, which, short, seq, ref, msn) {  // posFromRelativePos, mergeTree.ts:1371-1395
        if (!rp || typeof rp !== 'object') throw new UnsupportedError('relative position');
        const k = rp.id ? DocLog._idKey(rp.id) : null;
        if (k === null || !this.markerIds.has(k)) throw new UnsupportedError('relative position without a mapped marker (position -1)');
        if (this.markerDup.has(k) || this.markerIdAnnotated) {
            throw new UnsupportedError('relative position on a marker id remapped by block updates');
        }
        let off = rp.offset, flags = rp.before ? REL.BEFORE : 0;
        if (off !== undefined) {
            if (off === null) off = 0;  // pos += null adds 0
            if (typeof off !== 'number' || !Number.isInteger(off)) throw new UnsupportedError('relative position offset');
            flags |= REL.OFFSET;
        } else {
            off = 0;
        }
        this.push(OP.RELPOS, 0, short, seq, ref, msn, this.markerIds.get(k), which, off >>> 0, flags);
    }
    _position(op, key, which, short, seq, ref, msn) {  // op.pos1 / op.pos2, or its relativePos (client.ts:527-545)
        const v = op[key], rk = 'relative' + key[0].toUpperCase() + key.slice(1);
        if (v === undefined && op[rk]) {
            this._relpos(op[rk], which, short, seq, ref, msn);
            return 0;
        }
        if (typeof v !== 'number') throw new UnsupportedError('op without a usable ' + key);
        return Math.trunc(v);
    }
    shortId(longId) {  // Client.getOrAddShortClientId, client.ts:673-677
        const i = this.clientIx.get(longId);
        return i === undefined ? this.addLongId(longId) : i;
    }
    addLongId(longId) {  // Client.addLongClientId, client.ts:685-688: always a new short id
        if (this.clients.length >= MAX_CLIENTS) throw new UnsupportedError('more than ' + MAX_CLIENTS + ' client ids');
        const i = this.clients.length;
        this.clientIx.set(longId, i);
        this.clients.push(longId);
        return i;
    }
    _text(s) {
        const off = this.text.length;
        for (let i = 0; i < s.length; i++) this.text.push(s.charCodeAt(i));
        return [off, s.length];
    }
    _seg(spec, it, mapMarker = true) {  // specToSegment, sequence/src/sequenceFactory.ts:26-38 -> [flags, payload, payload2, propop]
        if (typeof spec === 'string') { const t = this._text(spec); return [0, t[0], t[1], -1]; }
        if (spec && typeof spec === 'object' && 'text' in spec) {
            const t = this._text(spec.text);
            if (spec.props !== undefined && spec.props !== null) return [F.PROPS, t[0], t[1], it.propop(spec.props)];
            return [0, t[0], t[1], -1];
        }
        if (spec && typeof spec === 'object' && 'marker' in spec) {
            const m = spec.marker || {};
            let flags = F.MARKER, ref = m.refType;
            if (ref === undefined || ref === null) { flags |= F.NOREF; ref = 0; }
            let pp = -1;
            if (spec.props !== undefined && spec.props !== null) { flags |= F.PROPS; pp = it.propop(spec.props); }
            return [flags, ref >>> 0, mapMarker ? this._mapMarker(spec.props) : 0, pp];
        }
        throw new UnsupportedError('unrecognized segment spec');
    }
    push(type, flags, client, seq, ref, msn, pos1, pos2, payload, payload2) {
        this.ops.push([type, flags, client, seq, ref, msn, pos1, pos2, payload, payload2]);
        this.nPushed = (this.nPushed || 0) + 1;  // (a stamp: getContainingSegment -> createLocalReferencePosition)
    }
    // local edits (client.ts:225-260): final before collaboration; while collaborating a pending op
    // (record seq = UnassignedSequenceNumber) until this client's sequenced message acks it
    localSeq() { return this.collaborating ? -1 : 0; }
    localInsert(pos, spec, it) {
        const s = this._seg(spec, it);
        this.push(OP.LOCAL_INSERT, s[0], 0, this.localSeq(), 0, 0, pos, s[3], s[1], s[2]);
    }
    localRemove(start, end) { this.push(OP.LOCAL_REMOVE, 0, 0, this.localSeq(), 0, 0, start, end, 0, 0); }
    // a local reference (localReference.ts): getContainingSegment(pos, view) [+ getSlideToSegment], then
    // createLocalReferencePosition -- view = {referenceSequenceNumber, clientId} or undefined (the local view)
    createRef(pos, refType, view, slide) {
        let short = 0, ref = 0, flags = REF.LOCALVIEW;
        if (view !== undefined) {
            const cid = view.clientId === null || view.clientId === undefined ? 'null' : String(view.clientId);
            short = this.shortId(cid);
            ref = view.referenceSequenceNumber;
            flags = 0;
        }
        if (slide) flags |= REF.SLIDE;
        const id = this._newRefId();
        this.push(OP.REF_CREATE, 0, short, 0, ref, 0, pos, id, refType, flags | REF.SLOT);
        return id;
    }
    _newRefId() { return this.freeRefs.length ? this.freeRefs.pop() : this.nRefs++; }
    removeRef(id) { this.push(OP.REF_REMOVE, 0, 0, 0, 0, 0, 0, 0, id, 0); }
    // the host is done with reference `id`: its id is reused by the next create (MTR_REF_SLOT); remove: a reference a
    // segment's collection may hold (a superseded or deleted interval endpoint) is removed first, a Transient query
    // reference needs no record (fluidframework_amd/batch.py DocLog.release_ref)
    releaseRef(id, remove = true) {
        if (!(id >= 0 && id < this.nRefs) || this.freeRefs.includes(id)) throw new Error('no local reference ' + id);
        if (remove) this.removeRef(id);
        this.freeRefs.push(id);
    }
    // createPositionReference with a localSeq (a rebase's changeInterval): getContainingSegment(pos, undefined,
    // localSeq) -- this client's view at (refSeq, localSeq) -- then createLocalReferencePosition
    createRefAt(pos, refType, refSeq, localSeq) {
        const id = this._newRefId();
        this.push(OP.REF_CREATE, 0, 0, 0, refSeq, localSeq, pos, id, refType, REF.LSEQ | REF.SLOT);
        return id;
    }
    ackRef(id) { this.push(OP.REF_ACK, 0, 0, 0, 0, 0, 0, 0, id, 0); }  // IntervalCollection.ackInterval, one endpoint
    // rebasePositionWithSegmentSlide(pos, seqNumberFrom, localSeq): returns the record index its result names
    rebasePosition(pos, seqFrom, localSeq) {
        this.push(OP.REBASE_POS, F.DELTA, 0, 0, seqFrom, localSeq, pos, 0, 0, 0);
        return this.ops.length - 1;
    }
    bumpLocalSeq() { this.push(OP.LSEQ, 0, 0, 0, 0, 0, 0, 0, 0, 0); }  // IntervalCollection.getNextLocalSeq
    localAnnotate(start, end, props, it, combiningOp) {
        if (props && typeof props === 'object' && 'markerId' in props) this.markerIdAnnotated = true;
        let comb = localComb(combiningOp), pp;
        if (comb === COMB.NONE || comb === COMB.REWRITE) {
            pp = it.propop(props);
        } else {  // combine(op, previousValue, undefined, seq): each key's absent-key result, as for a remote one
            const c = it.combining(props, combiningOp, this.collaborating ? -1 : 0);
            pp = c[0];
            comb = c[1];
        }
        this.push(OP.LOCAL_ANNOTATE, 0, 0, this.localSeq(), 0, 0, start, end, pp, comb);
    }
    rollback(op, it) {  // Client.rollback (client.ts:421-423 -> MergeTree.rollback, mergeTree.ts:2049-2159)
        let pp = 0, comb = 0;
        if (op.type === 2) {
            comb = localComb(op.combiningOp);
            pp = it.propop(op.props || {});
        } else if (op.type !== 0 && op.type !== 1) {
            throw new UnsupportedError('rollback of op type ' + op.type);
        }
        this.push(OP.ROLLBACK, 0, 0, -1, 0, 0, comb, 0, pp, op.type);
    }
    // Client.regeneratePendingOp (client.ts:917-960): one record per member op; returns the first record's
    // index in this batch (the op field of its MTR_DELTA_REGEN records)
    regenerate(op) {
        const members = op.type === 3 ? op.ops : [op];
        const first = this.ops.length;
        for (const m of members) {
            if (m.type !== 0 && m.type !== 1 && m.type !== 2) throw new UnsupportedError('regenerate of op type ' + m.type);
            this.push(OP.REGENERATE, F.DELTA, 0, -1, 0, 0, 0, 0, 0, m.type);
        }
        return first;
    }
    localOp(op, it) {  // Client.localTransaction member (client.ts:1029-1048)
        if (op.type === 0) this.localInsert(op.pos1, op.seg, it);
        else if (op.type === 1) this.localRemove(op.pos1, op.pos2);
        else if (op.type === 2) this.localAnnotate(op.pos1, op.pos2, op.props || {}, it, op.combiningOp);
        else throw new UnsupportedError('local op type ' + op.type);
    }
    startCollab(longId, minSeq, currentSeq) {  // client.ts:1133-1155
        if (longId === undefined) return;  // detached: stay local until attached
        if (this.observerId === undefined) {
            this.observerId = longId;
            const me = this.addLongId(longId);
            this.collaborating = true;
            this.currentSeq = currentSeq;
            this.push(OP.START_COLLAB, 0, me, currentSeq, 0, minSeq, 0, 0, 0, 0);
        } else {  // reconnect under a new id: the observer's short id is renamed
            const me = this.clientIx.get(this.observerId);
            this.observerId = longId;
            this.clientIx.set(longId, me);
            this.clients[me] = longId;
        }
    }
    seqUpdate(min, seq) { this.currentSeq = seq; this.push(OP.SEQ, F.LAST, 0, seq, seq, min, 0, 0, 0, 0); }
    // SnapshotLoader.specToSegment (snapshotLoader.ts:88-128): one LOAD (header) / APPEND (body) record whose
    // removedClientIds (short ids) ride in the text arena
    _snapshotSeg(spec, it, opType, flags) {
        // a loaded live marker is mapped by reloadFromSegments' blockUpdate (addNodeReferences, mergeTree.ts:297-306,
        // localNetLength > 0 only); a body segment by blockInsert (:1655-1662)
        const withInfo = spec !== null && typeof spec === 'object' && 'json' in spec;  // hasMergeInfo, snapshotChunks.ts:80-84
        const removed = withInfo && spec.removedSeq !== undefined && spec.removedSeq !== null;
        const live = opType !== OP.LOAD || !removed;
        let s, client = CLIENT_NONCOLLAB, seq = 0, removers = [], rseq = -1;
        if (withInfo) {
            s = this._seg(spec.json, it, live);
            if (spec.client !== undefined && spec.client !== null) client = this.shortId(spec.client);
            if (spec.seq !== undefined && spec.seq !== null) seq = spec.seq;
            if (spec.removedClient !== undefined && spec.removedClient !== null) removers = [this.shortId(spec.removedClient)];
            if (spec.removedClientIds !== undefined && spec.removedClientIds !== null) {
                removers = spec.removedClientIds.map((x) => this.shortId(x));
            }
            if (removed) rseq = spec.removedSeq;
        } else {
            s = this._seg(spec, it, live);
        }
        const roff = this.text.length;
        for (const r of removers) this.text.push(r);
        this.push(opType, s[0] | flags, client, seq, rseq, removers.length, roff, s[3], s[1], s[2]);
    }
    // Client.load -> SnapshotLoader.initialize (snapshotLoader.ts:41-257) from a summary's blobs {name: JSON text}:
    // header segments as reloadFromSegments records, startOrUpdateCollaboration(longId, minSeq, seq) (longId
    // undefined: a detached load stays local), body segments appended.  Returns the catch-up messages of a legacy
    // summary (the caller applies them as ordinary messages), [] otherwise.  Mirrors batch.py DocLog.load_summary.
    loadSummary(blobs, longId, it) {
        const chunk = JSON.parse(blobs.header);
        let segs, meta;
        if (chunk.version === '1') {
            segs = chunk.segments;
            meta = chunk.headerMetadata;
        } else {  // toLatestVersion of a legacy chunk, snapshotChunks.ts:151-200
            segs = chunk.segmentTexts;
            meta = chunk.headerMetadata || {
                orderedChunkMetadata: [{ id: 'header' }].concat(chunk.chunkLengthChars < chunk.totalLengthChars ? [{ id: 'body' }] : []),
                minSequenceNumber: chunk.chunkMinSequenceNumber,
                sequenceNumber: chunk.chunkSequenceNumber,
            };
        }
        if (meta === undefined) throw new Error('header metadata not available');
        for (const spec of segs) this._snapshotSeg(spec, it, OP.LOAD, 0);
        const minSeq = meta.minSequenceNumber;
        const seq = meta.sequenceNumber;
        this.startCollab(longId, minSeq !== undefined && minSeq !== null ? minSeq : seq, seq);
        for (const md of meta.orderedChunkMetadata.slice(1)) {
            if (blobs[md.id] === undefined) throw new Error('missing summary blob ' + md.id);
            const body = JSON.parse(blobs[md.id]);
            for (const spec of (body.segments !== undefined ? body.segments : (body.segmentTexts || []))) {
                this._snapshotSeg(spec, it, OP.INSERT, F.APPEND);
            }
        }
        const names = new Set(['header'].concat(meta.orderedChunkMetadata.map((md) => md.id)));
        const extra = Object.keys(blobs).filter((k) => !names.has(k));
        if (extra.length > 1) throw new Error('0x060');  // "There should be only one blob with catch up ops"
        return extra.length ? JSON.parse(blobs[extra[0]]) : [];
    }
    message(msg, it, local) {  // Client.applyMsg, client.ts:858-887
        const cid = msg.clientId === null || msg.clientId === undefined ? 'null' : String(msg.clientId);
        const short = this.shortId(cid);
        const seq = msg.sequenceNumber, ref = msg.referenceSequenceNumber, msn = msg.minimumSequenceNumber;
        if (msg.type !== 'op') { this.currentSeq = seq; this.push(OP.SEQ, F.LAST, short, seq, ref, msn, 0, 0, 0, 0); return; }
        let contents = msg.contents;
        if (typeof contents === 'string') contents = JSON.parse(contents);
        if (contents && contents.type === 'act') {  // an interval collection's op (sequence.ts:620-646): not a merge-tree op
            if (this.intervals === undefined) this.intervals = new IntervalCollections();
            this._intervals(() => this.intervals.process(this, contents, msg));
            return;
        }
        this.currentSeq = seq;
        const members = contents.type === 3 ? contents.ops : [contents];  // MergeTreeDeltaType.GROUP
        if (members.length === 0) { this.push(OP.SEQ, F.LAST, short, seq, ref, msn, 0, 0, 0, 0); return; }
        if (cid === this.observerId || local) {  // ackPendingSegment per member (client.ts:641-663, 866-869)
            members.forEach((op, i) => {
                const last = i === members.length - 1 ? F.LAST : 0;
                let pp = 0, comb = 0;
                if (op.type === 2) {
                    comb = localComb(op.combiningOp);
                    pp = it.propop(op.props || {});
                } else if (op.type !== 0 && op.type !== 1) {
                    throw new UnsupportedError('ack of op type ' + op.type);
                }
                this.push(OP.ACK, last, short, seq, ref, msn, comb, 0, pp, op.type);
            });
            return;
        }
        members.forEach((op, i) => {
            const last = i === members.length - 1 ? F.LAST : 0;
            if (op.type === 0) {
                if (op.seg === undefined || op.seg === null) {  // applyInsertOp returns early
                    this.push(OP.SEQ, last, short, seq, ref, msn, 0, 0, 0, 0);
                    return;
                }
                const n0 = this.ops.length;
                const pos1 = this._position(op, 'pos1', 1, short, seq, ref, msn);
                const rel = this.ops.length > n0 ? F.REL : 0;
                const s = this._seg(op.seg, it);
                this.push(OP.INSERT, s[0] | last | rel, short, seq, ref, msn, pos1, s[3], s[1], s[2]);
            } else if (op.type === 1) {
                const n0 = this.ops.length;
                const pos1 = this._position(op, 'pos1', 1, short, seq, ref, msn);
                const pos2 = this._position(op, 'pos2', 2, short, seq, ref, msn);
                const rel = this.ops.length > n0 ? F.REL : 0;
                this.push(OP.REMOVE, last | rel, short, seq, ref, msn, pos1, pos2, 0, 0);
            } else if (op.type === 2) {
                if (op.props && typeof op.props === 'object' && 'markerId' in op.props) this.markerIdAnnotated = true;
                const n0 = this.ops.length;
                const pos1 = this._position(op, 'pos1', 1, short, seq, ref, msn);
                const pos2 = this._position(op, 'pos2', 2, short, seq, ref, msn);
                const rel = this.ops.length > n0 ? F.REL : 0;
                const c = it.combining(op.props, op.combiningOp, seq);
                this.push(OP.ANNOTATE, last | rel, short, seq, ref, msn, pos1, pos2, c[0], c[1]);
            } else {
                throw new UnsupportedError('op type ' + op.type);
            }
        });
    }
}

/*
 * SharedMatrix (SharedMatrix.processCore, matrix/src/matrix.ts:636-693, remote branch): vector ops
 * (contents.target "rows" / "cols") are merge-tree ops on that PermutationVector, whose segment specs
 * are [length, start] (permutationvector.ts:45-48; the remote start is discarded on INSERT); a set-cell
 * message is one SETCELL record.  Both vectors share the rows log's client table.  Mirrors
 * fluidframework_amd/batch.py MatrixLog record for record.
 */
class MatrixDocLog extends DocLog {
    message(msg, it) {
        const cid = msg.clientId === null || msg.clientId === undefined ? 'null' : String(msg.clientId);
        if (msg.type !== 'op') return;  // SharedMatrix has no MSN handler of its own
        if (cid === this.observerId) throw new UnsupportedError('message authored by the observer (local ack path)');
        const short = this.shortId(cid);
        const seq = msg.sequenceNumber, ref = msg.referenceSequenceNumber, msn = msg.minimumSequenceNumber;
        let contents = msg.contents;
        if (typeof contents === 'string') contents = JSON.parse(contents);
        const target = contents.target;
        if (target === undefined || target === null) {  // MatrixOp.set (matrix/src/ops.ts:8-12)
            if (contents.type !== 2) throw new UnsupportedError('matrix message without a target');
            this.push(OP.SETCELL, 0, short, seq, ref, msn, contents.row, contents.col, 0, 0);
            return;
        }
        if (target !== 'rows' && target !== 'cols') throw new UnsupportedError('matrix target ' + target);
        const tf = target === 'cols' ? F.COLS : 0;
        const members = contents.type === 3 ? contents.ops : [contents];
        if (members.length === 0) { this.push(OP.SEQ, F.LAST | tf, short, seq, ref, msn, 0, 0, 0, 0); return; }
        members.forEach((op, i) => {
            const last = (i === members.length - 1 ? F.LAST : 0) | tf;
            if ('relativePos1' in op || 'relativePos2' in op) throw new UnsupportedError('relative positions');
            if (op.type === 0) {
                const seg = op.seg;
                if (seg === undefined || seg === null) { this.push(OP.SEQ, last, short, seq, ref, msn, 0, 0, 0, 0); return; }
                if (!Array.isArray(seg) || seg.length !== 2) throw new UnsupportedError('PermutationSegment spec');
                this.push(OP.INSERT, last, short, seq, ref, msn, op.pos1, -1, 0, seg[0]);
            } else if (op.type === 1) {
                this.push(OP.REMOVE, last, short, seq, ref, msn, op.pos1, op.pos2, 0, 0);
            } else {
                throw new UnsupportedError('vector op type ' + op.type);
            }
        });
    }
    colsLog() {  // the cols vector's engine document: no ops of its own, the same client table
        const c = new DocLog();
        c.observerId = this.observerId;
        c.clients = this.clients.slice();
        c.clientIx = new Map(this.clientIx);
        return c;
    }
}
/** Engine document order for matrices: [rows 0, cols 0, rows 1, cols 1, ...] (pair 2m / 2m+1). */
// blob ids as the addon takes them: a Buffer of 20-byte ids, from that or from an array of 40-digit hex strings
function idBuffer(ids) {
    if (Buffer.isBuffer(ids)) return ids;
    for (const id of ids) {
        if (typeof id !== 'string' || !/^[0-9a-fA-F]{40}$/.test(id)) throw new TypeError('a blob id is 40 hex digits');
    }
    return Buffer.from(ids.join(''), 'hex');
}

function matrixLogs(logs) {
    const out = [];
    for (const m of logs) { out.push(m); out.push(m.colsLog()); }
    return out;
}

function offsets(chunks) {
    const off = new Uint32Array(chunks.length + 1);
    for (let i = 0; i < chunks.length; i++) off[i + 1] = off[i] + chunks[i].length;
    return [off, Buffer.concat(chunks.concat([Buffer.alloc(1)]))];
}

/** Pack the queued ops of every DocLog (in order) into the arrays of include/mtr_types.h and clear them. */
function buildBatch(logs, it) {
    const nOps = logs.reduce((a, l) => a + l.ops.length, 0);
    const nText = logs.reduce((a, l) => a + l.text.length, 0);
    const docs = Buffer.alloc(32 * logs.length);
    const ops = Buffer.alloc(32 * nOps);
    const text = new Uint16Array(Math.max(1, nText));
    const clientChunks = [];
    let o = 0, t = 0;
    logs.forEach((log, d) => {
        const b = 32 * d;
        docs.writeUInt32LE(o >>> 0, b); docs.writeUInt32LE(Math.floor(o / 4294967296), b + 4);
        docs.writeUInt32LE(t >>> 0, b + 8); docs.writeUInt32LE(Math.floor(t / 4294967296), b + 12);
        docs.writeUInt32LE(log.ops.length, b + 16);
        docs.writeUInt32LE(log.text.length, b + 20);
        docs.writeUInt32LE(clientChunks.length, b + 24);
        docs.writeUInt32LE(log.clients.length, b + 28);
        log.clients.forEach((c) => clientChunks.push(utf8(JSON.stringify(c).slice(1, -1))));
        for (const r of log.ops) {
            const q = 32 * o;
            ops.writeUInt8(r[0], q); ops.writeUInt8(r[1], q + 1); ops.writeUInt16LE(r[2], q + 2);
            ops.writeInt32LE(r[3], q + 4); ops.writeInt32LE(r[4], q + 8); ops.writeInt32LE(r[5], q + 12);
            ops.writeInt32LE(r[6], q + 16); ops.writeInt32LE(r[7], q + 20);
            ops.writeUInt32LE(r[8] >>> 0, q + 24); ops.writeUInt32LE(r[9] >>> 0, q + 28);
            o++;
        }
        text.set(log.text, t);
        t += log.text.length;
        log.ops = []; log.text = [];
    });
    const po = new Uint32Array(it.propops.length + 1);
    const kv = [];
    it.propops.forEach((pairs, i) => { po[i + 1] = po[i] + pairs.length; pairs.forEach((p) => kv.push(p[0], p[1])); });
    const k = offsets(it.keyBytes), v = offsets(it.valBytes), c = offsets(clientChunks);
    return {
        docs, ops, text, propopOff: po, propopKv: Uint32Array.from(kv.length ? kv : [0]),
        keyOff: k[0], keyBytes: k[1], keyIndex: Uint32Array.from(it.keyIndex.length ? it.keyIndex : [0]),
        valOff: v[0], valBytes: v[1], valEq: Uint32Array.from(it.valEq.length ? it.valEq : [0]),
        clientOff: c[0], clientBytes: c[1],
    };
}

/*
 * Legacy-format catch-up messages (SURVEY.md §8 row f2).  SharedSegmentSequence keeps the messages
 * since the MSN and rewrites each lagging one (refSeq != seq - 1) from the sequenceDelta events its
 * application raised (createOpsFromDelta / processMergeTreeMsg, sequence.ts:120-173, 697-736).  The
 * engine applies messages in batches and raises no events, so the shim keeps that list itself: the
 * lagging message's ops are flagged F.DELTA, the engine reports each delta range (op, position in the
 * local view, cachedLength, kind; mtr_get_deltas) and the ops are rebuilt here after the batch.
 */
function sameProps(a, b) {  // matchProperties, properties.ts:71-105 (JS semantics, written out)
    if (!a) return !b;
    if (!b) return false;
    for (const k in a) {
        const y = b[k];
        if (y === undefined) return false;
        if (typeof y === 'object' ? !sameProps(a[k], y) : y !== a[k]) return false;
    }
    for (const k in b) if (a[k] === undefined) return false;
    return true;
}
function insertedSegmentJson(spec) {  // segment.clone().toJSONObject() of the segment an insert creates
    const kept = (p) => { const o = {}; Object.keys(p).forEach((k) => { if (p[k] !== null) o[k] = p[k]; }); return o; };
    if (typeof spec === 'string') return spec;
    const hasProps = spec.props !== undefined && spec.props !== null;
    if ('text' in spec) return hasProps ? { text: spec.text, props: kept(spec.props) } : spec.text;
    const m = spec.marker || {};
    const out = { marker: m.refType === undefined || m.refType === null ? {} : { refType: m.refType } };
    if (hasProps) out.props = kept(spec.props);
    return out;
}
function opsFromDeltas(members, opIndex, byOp) {
    const ops = [];
    members.forEach((member, i) => {
        for (const r of byOp.get(opIndex[i]) || []) {
            const pos = r[1], len = r[2], last = ops.length ? ops[ops.length - 1] : undefined;
            if (r[3] === OP.ANNOTATE) {  // an observer's propertyDeltas hold every key of the op
                const props = {};
                Object.keys(member.props).forEach((k) => { props[k] = member.props[k]; });
                if (last && last.pos2 === pos && sameProps(last.props, props)) last.pos2 += len;
                else ops.push({ pos1: pos, pos2: pos + len, props, type: 2 });
            } else if (r[3] === OP.INSERT) {
                ops.push({ pos1: pos, seg: insertedSegmentJson(member.seg), type: 0 });
            } else if (r[3] === OP.REMOVE) {
                if (last && last.pos1 === pos) {
                    if (last.pos2 === undefined) throw new Error('0x3ff');  // sequence.ts:155-158
                    last.pos2 += len;
                } else {
                    ops.push({ pos1: pos, pos2: pos + len, type: 1 });
                }
            }
        }
    });
    return ops;
}
class CatchUpLog {
    constructor() { this.stash = []; this.pending = []; }
    /** After log.message(msg) queued the message's records from op index `lo` on. */
    add(msg, log, lo, own) {
        const copy = JSON.parse(JSON.stringify(msg));  // parseHandles (sequence.ts:698)
        if (typeof copy.contents === 'string') copy.contents = JSON.parse(copy.contents);
        if (own && copy.referenceSequenceNumber !== copy.sequenceNumber - 1) {
            // an ack raises no "delta" event (ackPendingSegment, mergeTree.ts:1283-1323): transformOps collects
            // nothing and the stashed copy is createGroupOp() of no ops (sequence.ts:697-725, opBuilder.ts:102-107)
            copy.referenceSequenceNumber = copy.sequenceNumber - 1;
            copy.contents = { ops: [], type: 3 };
        } else if (copy.referenceSequenceNumber !== copy.sequenceNumber - 1) {
            const members = copy.contents.type === 3 ? copy.contents.ops : [copy.contents];
            const opIndex = members.map((_, i) => {
                const r = log.ops[lo + i];
                if (r[0] !== OP.INSERT && r[0] !== OP.REMOVE && r[0] !== OP.ANNOTATE) return -1;
                r[1] |= F.DELTA;
                return lo + i;
            });
            copy.referenceSequenceNumber = copy.sequenceNumber - 1;
            this.pending.push({ msg: copy, members, opIndex });
        }
        this.stash.push(copy);
        if (this.stash.length > 20 && this.stash[20].sequenceNumber < msg.minimumSequenceNumber) {
            this.trim(msg.minimumSequenceNumber);  // sequence.ts:728-734
        }
    }
    resolve(deltas) {  // Int32Array of [op, pos, len, kind] records of the batch just applied
        const byOp = new Map();
        for (let i = 0; i < deltas.length; i += 4) {
            const r = [deltas[i], deltas[i + 1], deltas[i + 2], deltas[i + 3]];
            if (!byOp.has(r[0])) byOp.set(r[0], []);
            byOp.get(r[0]).push(r);
        }
        for (const p of this.pending) {
            const ops = opsFromDeltas(p.members, p.opIndex, byOp);
            p.msg.contents = ops.length === 1 ? ops[0] : { ops, type: 3 };  // createGroupOp
        }
        this.pending = [];
    }
    trim(minSeq) {  // processMinSequenceNumberChanged, sequence.ts:738-748
        let i = 0;
        while (i < this.stash.length && this.stash[i].sequenceNumber <= minSeq) i++;
        if (i) this.stash = this.stash.slice(i);
    }
    forSummary(minSeq) {  // summarizeMergeTree, sequence.ts:675-695
        this.trim(minSeq);
        this.stash.forEach((m) => { m.minimumSequenceNumber = minSeq; });
        return this.stash;
    }
}

/** The observer Clients of many documents on one GPU. */
/*
 * resetPendingDeltaToOps (client.ts:708-800) from the engine's MTR_DELTA_REGEN / _X record pairs
 * (include/mtr_types.h): per member of the pending group, in tree order, the op to resubmit --
 * createInsertSegmentOp (the member's piece of the text, the op's own seg.props or else the segment's
 * current properties), createRemoveRangeOp, createAnnotateRangeOp -- and a GROUP unless exactly one.
 * The Python mirror is fluidframework_amd/regen.py.
 */
function regenRecords(d) {  // Int32Array of [op, pos, len, kind] -> Map(record index -> [[type, pos, len, off, ref]])
    const out = new Map();
    for (let i = 0; i < d.length; i += 4) {
        const kind = d[i + 3] >>> 0;
        if (kind < DELTA_REGEN || kind >= DELTA_REGEN + 3) continue;
        if (i + 4 >= d.length || (d[i + 7] >>> 0) !== DELTA_REGEN_X) throw new Error('MTR_DELTA_REGEN without its _X record');
        const op = d[i] >>> 0;
        if (!out.has(op)) out.set(op, []);
        out.get(op).push([kind - DELTA_REGEN, d[i + 1], d[i + 2], d[i + 5], d[i + 6]]);
        i += 4;
    }
    return out;
}
function regenMember(op, r, propsOf) {
    const [t, pos, n, off, ref] = r;
    if (t !== op.type) throw new Error('regenerate record does not match the op');
    if (t === 1) return { pos1: pos, pos2: pos + n, type: 1 };
    if (t === 2) {
        const o = { pos1: pos, pos2: pos + n, props: op.props, type: 2 };
        if (op.combiningOp !== undefined) o.combiningOp = op.combiningOp;
        return o;
    }
    const seg = op.seg;
    const own = seg !== null && typeof seg === 'object' && seg.props !== undefined;  // client.ts:763-767
    const props = own ? seg.props : (ref >= 0 ? propsOf(ref) : undefined);
    let spec;
    if (seg !== null && typeof seg === 'object' && 'marker' in seg) {
        spec = { marker: seg.marker };
        if (props !== undefined && props !== null) spec.props = props;
    } else {
        const text = (typeof seg === 'string' ? seg : seg.text).substring(off, off + n);  // UTF-16 units
        spec = props !== undefined && props !== null ? { text, props } : text;
    }
    return { pos1: pos, seg: spec, type: 0 };
}
function regeneratedOp(resetOp, recs, first, propsOf) {
    const members = resetOp.type === 3 ? resetOp.ops : [resetOp];
    const ops = [];
    members.forEach((m, k) => { for (const r of recs.get(first + k) || []) ops.push(regenMember(m, r, propsOf)); });
    return ops.length === 1 ? ops[0] : { ops, type: 3 };
}

// a local annotate's combiningOp: none or "rewrite" (pendingRewriteCount, segmentPropertiesManager.ts:72-80); its
// ack and rollback records carry the same code (pos1)
function localComb(co) {  // a local annotate's combiningOp as its ack / rollback records carry it (batch.py _local_comb)
    if (!co) return COMB.NONE;
    if (typeof co !== 'object') throw new UnsupportedError('combiningOp');
    if (co.name === 'rewrite') return COMB.REWRITE;
    return co.name === 'incr' ? COMB.INCR : co.name === 'consensus' ? COMB.CONSENSUS : COMB.KEEP;
}

class BatchReplayEngine {
    constructor(maxDocs, options) {
        this.options = Object.assign({ newLengthCalc: 0, snapshotV1: 1, chunkSize: 10000, device: 0 }, options || {});
        this.maxDocs = maxDocs;
        this.h = native().createEngine(maxDocs, this.options);
        this.interner = new Interner();
        this.logs = [];
        this.catchUps = [];
        this.dirty = false;
        this.summarized = false;
        this.inFlight = false;  // an async run / summarize holds the engine (its batch was taken from the logs)
    }
    _assertIdle() {
        if (this.inFlight) throw new Error('engine busy: await the pending flushAsync / summarizeAllAsync first');
    }
    createClient() {
        if (this.logs.length >= this.maxDocs) throw new Error('engine is full');
        this.logs.push(new DocLog());
        this.catchUps.push(new CatchUpLog());
        return new BatchReplayClient(this, this.logs.length - 1);
    }
    createMatrix() {  // a SharedMatrix: its rows and cols PermutationVectors as engine documents 2k, 2k+1
        if (this.logs.length + 2 > this.maxDocs) throw new Error('engine is full');
        const rows = this.logs.length;
        const log = new MatrixDocLog();
        this.logs.push(log, log.colsLog());
        this.catchUps.push(new CatchUpLog(), new CatchUpLog());
        native().setMatrix(this.h, rows, rows + 1);
        return new BatchMatrixClient(this, rows);
    }
    _batch() {
        this.logs.forEach((l, d) => {  // cols vectors share their rows log's client table
            if (l instanceof MatrixDocLog) this.logs[d + 1] = l.colsLog();
        });
        return buildBatch(this.logs, this.interner);
    }
    _afterRun() {
        // the documents with pending catch-ups, their delta records from one batched call
        const docs = [];
        this.catchUps.forEach((c, d) => { if (c.pending.length) docs.push(d); });
        if (docs.length) {
            const r = native().getDeltasBatch(this.h, Uint32Array.from(docs), docs.length, false);
            docs.forEach((d, i) => this.catchUps[d].resolve(r.records.subarray(4 * r.docFirst[i], 4 * r.docFirst[i + 1])));
        }
        this.dirty = false;
        this.summarized = false;
    }
    flush() {  // apply every queued message of every document
        this._assertIdle();
        if (!this.dirty) return;
        native().submitRun(this.h, this._batch());
        this._afterRun();
    }
    /**
     * The asynchronous flush: the batch is applied on a worker thread (N-API async work) and the
     * returned promise settles when the GPU is done, so the event loop keeps serving meanwhile.  Every
     * other call on this engine or its clients throws until it settles (await it): the batch has already
     * been taken from the logs, so nothing may be queued behind it.
     */
    async flushAsync() {
        this._assertIdle();
        if (!this.dirty) return;
        const batch = this._batch();
        this.inFlight = true;
        try {
            await native().submitRunAsync(this.h, batch);
        } finally {
            this.inFlight = false;
        }
        this._afterRun();
    }
    /**
     * BatchReplayClient.getContainingSegment for many views of many documents in one batched call
     * (mtr_get_containing_segments: one launch, a workgroup per query).  queries: [{client, pos, sequenceArgs}] with
     * client a BatchReplayClient of this engine; -> getContainingSegment's result objects, one per query in order.
     */
    getContainingSegments(queries) {
        this.flush();
        const w = new Int32Array(4 * queries.length);
        queries.forEach((q, i) => {
            if (!(q.client instanceof BatchReplayClient) || q.client.engine !== this) {
                throw new Error(`getContainingSegments: query ${i} names no client of this engine`);
            }
            q.client._check();
            const [ref, client] = q.client._viewOf(q.sequenceArgs);
            w.set([q.client.doc, q.pos, ref, client], 4 * i);
        });
        const res = native().getContainingSegments(this.h, w);
        return queries.map((q, i) => q.client._containing(res[i], q.sequenceArgs));
    }
    /** the queries of getRangeSegments / getTextRanges as the addon takes them: [doc, start, end, refSeq, client] * n */
    _rangeWords(name, queries) {
        this.flush();
        const w = new Int32Array(5 * queries.length);
        queries.forEach((q, i) => {
            if (!(q.client instanceof BatchReplayClient) || q.client.engine !== this) {
                throw new Error(`${name}: query ${i} names no client of this engine`);
            }
            q.client._check();
            const [ref, client] = q.client._viewOf(q.sequenceArgs);
            w.set([q.client.doc, q.start === undefined ? 0 : q.start, q.end === undefined ? 0x7fffffff : q.end, ref, client], 5 * i);
        });
        return w;
    }
    /**
     * Client.walkSegments(handler, start, end) for many ranges of many documents in one batched call
     * (mtr_get_range_segments: a wave per query).  queries: [{client, start, end, sequenceArgs}] with client a
     * BatchReplayClient of this engine (start default 0, end default the view's end); placeholder: one character a
     * marker's text is, default none.  -> per query the list of getContainingSegment's results for its segments in
     * order: the first one's offset is the clip at `start`, and a text segment's text holds its units inside the range.
     */
    getRangeSegments(queries, placeholder) {
        const w = this._rangeWords('getRangeSegments', queries);
        const res = native().getRanges(this.h, w, placeholder ? placeholder.charCodeAt(0) : 0, true);
        return queries.map((q, i) => res.segments.slice(res.segFirst[i], res.segFirst[i + 1])
            .map((r) => q.client._containing(r, q.sequenceArgs)));
    }
    /**
     * getText(refSeq, clientId, placeholder, start, end) (MergeTreeTextHelper.ts:20-81) for many ranges in one batched
     * call: the text-only form of getRangeSegments (no segment rows are built or downloaded).  -> one string per query.
     */
    getTextRanges(queries, placeholder) {
        const w = this._rangeWords('getTextRanges', queries);
        const res = native().getRanges(this.h, w, placeholder ? placeholder.charCodeAt(0) : 0, false);
        return queries.map((q, i) => res.text.slice(res.textFirst[i], res.textFirst[i + 1]));
    }
    /** mtr_transform_positions over rows of [doc, pos, refSeq, client, toRefSeq, toClient, mode, offset] -> Int32Array
     *  of [pos, leaf, offset, flags] per row */
    _transform(rows) {
        const w = new Int32Array(8 * rows.length);
        rows.forEach((r, i) => w.set(r, 8 * i));
        return native().transformPositions(this.h, w.buffer);
    }
    /**
     * Client.resolveRemoteClientPosition(remotePos, remoteRefSeq, remoteClientId) (client.ts) for many positions of
     * many documents in one batched call (mtr_transform_positions: one launch, a wave per query).  queries: [{client,
     * pos, sequenceArgs}] with client a BatchReplayClient of this engine and sequenceArgs = {referenceSequenceNumber,
     * clientId} the remote view pos is a position of; -> per query the position in that client's own current view, or
     * undefined where the remote view holds no such position.
     */
    resolveRemoteClientPositions(queries) {
        this.flush();
        const rows = queries.map((q, i) => {
            if (!(q.client instanceof BatchReplayClient) || q.client.engine !== this) {
                throw new Error(`resolveRemoteClientPositions: query ${i} names no client of this engine`);
            }
            q.client._check();
            const [ref, client] = q.client._viewOf(q.sequenceArgs);
            const [toRef, toClient] = q.client._viewOf(undefined);
            return [q.client.doc, q.pos, ref, client, toRef, toClient, POS_FROM_VIEW, 0];
        });
        const res = this._transform(rows);
        return queries.map((q, i) => (res[4 * i] < 0 ? undefined : res[4 * i]));
    }
    /** mtr_find_markers' rows (6 words a query) -> {pos, leaf, refType, props, seq} per query, undefined where none */
    static _markerHits(res, n) {
        const out = [];
        for (let i = 0; i < n; i++) {
            const r = res.subarray(6 * i, 6 * i + 6);
            out.push(r[5] & MK_FOUND ? { pos: r[0], leaf: r[1], refType: r[2], props: r[3], seq: r[4] } : undefined);
        }
        return out;
    }
    /**
     * SharedString.findTile(pos, label, preceding) for many positions of many documents in one read-only batched call
     * (mtr_find_markers: one launch, a wave per query).  queries: [{client, pos, refSeq, clientId, label, preceding}]
     * with client a BatchReplayClient of this engine; refSeq / clientId name the view (default: that client's own
     * current view), preceding defaults to true.  -> per query {pos, leaf, refType, props, seq} of the nearest marker
     * at or before (preceding) or at or after pos whose referenceTileLabels hold the label, undefined where there is
     * none.
     */
    findTiles(queries) {
        this.flush();
        const labels = [], vals = [], index = new Map();
        const q = new Int32Array(6 * queries.length);
        queries.forEach((x, i) => {
            if (!(x.client instanceof BatchReplayClient) || x.client.engine !== this) {
                throw new Error(`findTiles: query ${i} names no client of this engine`);
            }
            x.client._check();
            const own = x.refSeq === undefined && x.clientId === undefined;
            const [ref, client] = x.client._viewOf(own ? undefined
                : { referenceSequenceNumber: x.refSeq === undefined ? x.client.currentSeq : x.refSeq, clientId: x.clientId });
            if (!index.has(x.label)) {
                const [key, ids] = this.interner.labelValues(TILE_LABELS_KEY, x.label);
                index.set(x.label, labels.length);
                // (a key no batch ever held comes with no values: a label without values matches nothing)
                labels.push([key === undefined ? 0 : key, vals.length, ids.length]);
                vals.push(...ids);
            }
            q.set([x.client.doc, x.pos, ref, client, x.preceding === false ? MK_FOLLOWING : MK_PRECEDING,
                index.get(x.label)], 6 * i);
        });
        const lb = new Uint32Array(3 * labels.length);
        labels.forEach((l, j) => lb.set(l, 3 * j));
        const res = native().findMarkers(this.h, lb.buffer, new Uint32Array(vals).buffer, q.buffer);
        return BatchReplayEngine._markerHits(res, queries.length);
    }
    /**
     * Interval queries over many collections of many documents from one read-only batched call (mtr_query_intervals:
     * no Transient reference is created).  sets: [{doc, first, count}]; refs: [[startRef, endRef]] per interval;
     * queries: [{set, start, end, mode}] with mode 0 overlap, 1 previous, 2 next -> {hitFirst: Float64Array [n + 1],
     * status: Int32Array [n] (1: an endpoint of the set on a segment zamboni took out of the tree), hits: Int32Array of
     * 8 words a hit: interval, startPos, endPos, startKey, startOff, endKey, endOff, flags (1: several intervals share
     * that end)}.
     */
    queryIntervals(sets, refs, queries) {
        this.flush();
        const s = new Uint32Array(3 * sets.length), r = new Uint32Array(2 * refs.length), q = new Int32Array(4 * queries.length);
        sets.forEach((x, i) => s.set([x.doc, x.first, x.count], 3 * i));
        refs.forEach((x, i) => r.set(x, 2 * i));
        queries.forEach((x, i) => q.set([x.set, x.start, x.end === undefined ? x.start : x.end, x.mode], 4 * i));
        return native().queryIntervals(this.h, s.buffer, r.buffer, q.buffer);
    }
    /**
     * The local references of many clients' documents from one batched call (mtr_get_refs: one launch for every
     * document, a wave per 64 references).  clients: BatchReplayClients of this engine in any order, repeats allowed;
     * mode: 1, 2 or 4 words per reference -- what getRefPositions, getRefStates and refKeys return for one document.
     * -> {docFirst, words}: client i's words are words[mode * docFirst[i] .. mode * docFirst[i + 1]).
     */
    getRefsBatch(clients, mode) {
        this.flush();
        const docs = new Uint32Array(clients.length);
        clients.forEach((c, i) => {
            if (!(c instanceof BatchReplayClient) || c.engine !== this) {
                throw new Error(`getRefsBatch: entry ${i} is no client of this engine`);
            }
            c._check();
            docs[i] = c.doc;
        });
        return native().getRefsBatch(this.h, docs, docs.length, mode);
    }
    /**
     * The delta records of many clients' documents from one batched call (mtr_get_deltas_batch: a wave per document,
     * 64 records a round).  clients: BatchReplayClients of this engine in any order, repeats allowed.
     * -> {docFirst, records}: client i's [op, pos, len, kind] records are records[4 * docFirst[i] ..
     * 4 * docFirst[i + 1]); with wantProps also {propsOff, props}: record r's property words (what getProps returns
     * for an MTR_DELTA_REGEN_X record) are props[propsOff[r] .. propsOff[r + 1]).
     */
    getDeltasBatch(clients, wantProps) {
        this.flush();
        const docs = new Uint32Array(clients.length);
        clients.forEach((c, i) => {
            if (!(c instanceof BatchReplayClient) || c.engine !== this) {
                throw new Error(`getDeltasBatch: entry ${i} is no client of this engine`);
            }
            c._check();
            docs[i] = c.doc;
        });
        return native().getDeltasBatch(this.h, docs, docs.length, !!wantProps);
    }
    /**
     * The summarizer's hand-over in one call (mtr_replay_pipelined through the addon's replaySummaries): every
     * queued message applied, every document summarized and its records in host memory -- document d's record is
     * bytes[docOff[d], docOff[d + 1]) = u32 blob count, u32 blob lengths, the blobs.  A batch of remote messages
     * goes through the pipelined path (ranges applied as they land, summarized and downloaded as they finish;
     * `pipelined` true), any other the serial calls.
     */
    replaySummaries(parts = 16) {
        this._assertIdle();
        const r = native().replaySummaries(this.h, this._batch(), parts);
        this._afterRun();
        this.summarized = true;
        return r;
    }
    /**
     * replaySummaries that downloads only the blobs storage lacks (mtr_replay_handover through the addon's
     * replayHandover): every queued message applied, every document summarized, and every blob of every document
     * sorted against the blob-id cache as summaryNovel() returns it -- blobs[k] = {id, state, rep, bytes?}; document
     * d's blobs are blobs[docFirst[d] .. docFirst[d + 1]).  A batch of remote messages goes through the pipelined path
     * (each range hashed, classified and gathered on the device as it finishes, the state-1 bytes alone downloaded;
     * `pipelined` true), any other the serial calls, with the same result.  The summary, its ids and the novel result
     * stay on the device: summaryTreeIds() and blobCacheAddSummary() follow without hashing again.
     */
    replayHandover(parts = 16) {
        this._assertIdle();
        const r = native().replayHandover(this.h, this._batch(), parts);
        this._afterRun();
        this.summarized = true;
        const blobs = r.ids.map((id, k) => (r.state[k] === 1 ? { id, state: 1, rep: r.rep[k], bytes: r.bytes[k] }
            : { id, state: r.state[k], rep: r.rep[k] }));
        return { blobs, docFirst: r.docFirst, pipelined: r.pipelined };
    }
    _summarizeAll() {
        this.flush();
        if (!this.summarized) { native().summarize(this.h); this.summarized = true; }
    }
    /**
     * The incremental hand-over.  markSummaryBaseline(): the git blob ids of the current summary (every queued
     * message applied, summarized if needed) become the baseline -- call it once storage has acknowledged the
     * upload.  The baseline is keyed by (document, blob index) and stays until it is marked again or cleared.
     */
    markSummaryBaseline() {
        this._assertIdle();
        this._summarizeAll();
        native().setSummaryBaseline(this.h);
    }
    clearSummaryBaseline() {
        this._assertIdle();
        native().clearSummaryBaseline(this.h);
    }
    /**
     * Every blob of documents [lo, hi) in record order (header, body / body_0, ...): ids[k] its git blob id,
     * changed[k] its bytes when it is new or differs from the baseline, null when the baseline holds the same id at
     * the same (document, index) -- refer to that blob by its id.  Document lo + i's blobs are
     * [docFirst[i], docFirst[i + 1]).  The changed blobs are gathered on the device and come over in one copy
     * (mtr_summary_delta).  Without a baseline every blob is changed.
     */
    summaryDelta(lo = 0, hi = this.logs.length) {
        this._assertIdle();
        this._summarizeAll();
        return native().summaryDelta(this.h, lo, hi);
    }
    /**
     * The blob-id cache: the set of git blob ids storage holds, under any path of any document, kept on the device --
     * the stand-in for SummaryTreeUploadManager's blobsShaCache.  It stays across batches, summaries and resets until
     * blobCacheClear().  ids: an array of 40-digit hex strings, or a Buffer of 20-byte ids.
     */
    blobCacheAdd(ids) {
        this._assertIdle();
        native().blobCacheAdd(this.h, idBuffer(ids));
    }
    /** The ids of the current summary (every queued message applied, summarized if needed) join the cache: call it
     * once storage has acknowledged the upload. */
    blobCacheAddSummary() {
        this._assertIdle();
        this._summarizeAll();
        native().blobCacheAddSummary(this.h);
    }
    blobCacheClear() {
        this._assertIdle();
        native().blobCacheClear(this.h);
    }
    blobCacheSize() {
        this._assertIdle();
        return native().blobCacheSize(this.h);
    }
    /** Per id: does the cache hold it -- for the blobs the host makes itself (catch-up ops, interval headers). */
    blobCacheHas(ids) {
        this._assertIdle();
        return native().blobCacheHas(this.h, idBuffer(ids));
    }
    /**
     * The cache's life cycle.  Every entry carries the generation at which its id was last offered; blobCacheAdd
     * stamps with the current generation, blobCacheAddSummary moves to the next one first (one acknowledged summary
     * is one generation).  blobCacheGeneration(): the current generation.
     */
    blobCacheGeneration() {
        this._assertIdle();
        return native().blobCacheGeneration(this.h);
    }
    /** ages[a] = the entries last referenced a generations ago; ages[n - 1] holds all older ones (1 <= n <= 1024). */
    blobCacheAges(n) {
        this._assertIdle();
        return native().blobCacheAges(this.h, n);
    }
    /** Drops the entries not referenced since minGeneration, on the device; returns how many.  The rest keep their
     * order. */
    blobCacheTrim(minGeneration) {
        this._assertIdle();
        return native().blobCacheTrim(this.h, minGeneration);
    }
    /** Trims to at most maxEntries entries by whole generations, oldest first; returns the entries removed. */
    blobCacheTrimTo(maxEntries) {
        this._assertIdle();
        return native().blobCacheTrimTo(this.h, maxEntries);
    }
    /** {ids: Buffer of 20-byte ids in table order, ages: number[]}: what blobCacheImport of a restarted summarizer
     * takes. */
    blobCacheExport() {
        this._assertIdle();
        return native().blobCacheExport(this.h);
    }
    /** Offers ids (hex strings or a Buffer) with their ages: the generation becomes at least the largest age, and of
     * equal ids the youngest age wins.  Importing an export into a fresh engine reproduces the cache. */
    blobCacheImport(ids, ages) {
        this._assertIdle();
        native().blobCacheImport(this.h, idBuffer(ids), Uint32Array.from(ages));
    }
    /**
     * Every blob of documents [lo, hi) in record order against the cache, as {id, state, rep, bytes?}: state 0 the
     * cache holds the id (refer to it by id); state 1 it is new and this is the first blob of the whole summary with
     * that id -- bytes holds it, upload it; state 2 it is new but blob `rep` (an index over all documents' blobs) of
     * this summary is the same object.  rep is the blob's own summary-wide index for state 1 and -1 for state 0.  The
     * state-1 blobs are gathered on the device and come over in one copy (mtr_summary_novel).
     */
    summaryNovel(lo = 0, hi = this.logs.length) {
        this._assertIdle();
        this._summarizeAll();
        const r = native().summaryNovel(this.h, lo, hi);
        return r.ids.map((id, k) => (r.state[k] === 1 ? { id, state: 1, rep: r.rep[k], bytes: r.bytes[k] }
            : { id, state: r.state[k], rep: r.rep[k] }));
    }
    /**
     * The git tree id (40 hex digits) of the summary tree of every document of [lo, hi): what storage answers
     * createGitTree with for the tree summarize() returns (SummaryTreeUploadManager.writeSummaryTreeCore), computed on
     * the device (mtr_summary_tree_ids) -- so an unchanged document is known by one 20-byte compare, and a tree seen
     * before needs no round trip.  extras[i]: the host-made entries of document lo + i's tree, each
     * {name, id, tree?: true for a subtree} (the legacy catch-up blob, an interval collection's header).
     */
    summaryTreeIds(lo = 0, hi = this.logs.length, extras = undefined) {
        this._assertIdle();
        this._summarizeAll();
        return extras === undefined ? native().summaryTreeIds(this.h, lo, hi) : native().summaryTreeIds(this.h, lo, hi, extras);
    }
    async summarizeAllAsync() {  // every document's blobs, built on a worker thread
        await this.flushAsync();
        if (!this.summarized) {
            this._assertIdle();
            this.inFlight = true;
            try {
                await native().summarizeAsync(this.h);
            } finally {
                this.inFlight = false;
            }
            this.summarized = true;
        }
    }
}

/** Client (client.ts:98) restricted to the observer path, backed by one engine document. */
class BatchReplayClient {
    constructor(engine, doc) {
        this.engine = engine; this.doc = doc; this.log = engine.logs[doc];
        this.currentSeq = 0;
        this.localSeq = 0;          // collabWindow.localSeq as this host counts it (interval ops too)
        this.lastNormalization = 0; // Client.lastNormalizationRefSeq (client.ts:910)
        this.emitters = new Map();  // label -> the collection's op emitter (IValueOpEmitter)
    }
    _queue(fn) { this.engine._assertIdle(); fn(); this.engine.dirty = true; }
    _check() {
        const st = native().docStatus(this.engine.h, this.doc);
        if (st[0] === STATUS.OK) return;
        if (st[0] >= STATUS.ASSERT) {  // assert(cond, 0xNNN) throws Error("0xNNN"), common-utils assert.ts:15-21
            throw new Error('0x' + (st[0] - STATUS.ASSERT).toString(16).padStart(3, '0'));
        }
        if (st[0] === STATUS.INSERT_FAILED) throw new Error('MergeTree insert failed');  // mergeTree.ts:1671
        if (st[0] === STATUS.UNSUPPORTED) throw new UnsupportedError('unsupported op at ' + st[1]);
        throw new Error('engine status ' + st[0] + ' at op ' + st[1]);
    }
    startOrUpdateCollaboration(longClientId, minSeq, currentSeq) {
        this._queue(() => this.log.startCollab(longClientId, minSeq || 0, currentSeq || 0));
        this.currentSeq = currentSeq || 0;
    }
    /**
     * Client.load (client.ts:1007-1019 -> SnapshotLoader.initialize, snapshotLoader.ts:41-257): the document
     * resumes from a merge-tree summary read through `storage` (IChannelStorageService: readBlob(path) ->
     * Buffer / Uint8Array, list(path) -> blob names).  A runtime that is not Detached starts collaboration as
     * runtime.clientId ?? "snapshot".  Resolves to {catchupOpsP}: the legacy format's catch-up messages, which
     * the caller applies with applyMsg (SharedSegmentSequence.loadCore does), [] for V1.
     */
    async load(runtime, storage, serializer) {
        const names = await storage.list('');
        const blobs = {};
        for (const n of names) {
            const b = await storage.readBlob(n);
            blobs[n] = typeof b === 'string' ? b : Buffer.from(b.buffer, b.byteOffset, b.byteLength).toString('utf8');
        }
        if (blobs.header === undefined) throw new Error('0x05f');  // "Missing blob header on legacy snapshot!"
        const detached = runtime && runtime.attachState === 'Detached';
        const longId = detached ? undefined : ((runtime && runtime.clientId) || 'snapshot');
        let catchup = [];
        this._queue(() => { catchup = this.log.loadSummary(blobs, longId, this.engine.interner); });
        const meta = JSON.parse(blobs.header);
        this.currentSeq = meta.version === '1' ? meta.headerMetadata.sequenceNumber
            : (meta.headerMetadata ? meta.headerMetadata.sequenceNumber : meta.chunkSequenceNumber);
        if (serializer && typeof serializer.parse === 'function' && catchup.length) {
            catchup = serializer.parse(JSON.stringify(catchup));
        }
        return { catchupOpsP: Promise.resolve(catchup) };
    }
    /** load from an ISummaryTree this shim (or the reference) produced: {type: Tree, tree: {name: {content}}}. */
    loadSummaryTree(summary, longClientId) {
        const blobs = {};
        for (const k of Object.keys(summary.tree)) {
            const c = summary.tree[k].content;
            blobs[k] = typeof c === 'string' ? c : Buffer.from(c).toString('utf8');
        }
        let catchup = [];
        this._queue(() => { catchup = this.log.loadSummary(blobs, longClientId, this.engine.interner); });
        return catchup;
    }
    applyMsg(msg, local, localOpMetadata) {
        const own = local || (msg.type === 'op' && String(msg.clientId) === this.log.observerId);
        if (msg.type === 'op' && this.log.collaborating && this.log.intervals !== undefined) {
            const c = typeof msg.contents === 'string' ? JSON.parse(msg.contents) : msg.contents;
            if (c && c.type === 'act' && (own || this.log.intervals.live)) {  // a live client's interval op
                this.processIntervalOp(msg, !!own, localOpMetadata);
                this.currentSeq = this.log.currentSeq;
                return;
            }
        }
        this._queue(() => {
            if (!this.engine.options.snapshotV1 && msg.type === 'op' && !own &&
                msg.referenceSequenceNumber !== msg.sequenceNumber - 1) {
                let c = msg.contents;
                if (typeof c === 'string') c = JSON.parse(c);
                for (const m of c.type === 3 ? (c.ops || []) : [c]) {
                    // the catch-up transform needs each member's post-op values / one record per member
                    if (m.combiningOp || m.relativePos1 || m.relativePos2) {
                        throw new UnsupportedError('a lagging message with a combining annotate or a relative position ' +
                            'in the legacy format');
                    }
                }
            }
            const lo = this.log.ops.length;
            this.log.message(msg, this.engine.interner, local);
            // (an interval op is handled by the collections and kept by no catch-up list, sequence.ts:636-645)
            if (!this.engine.options.snapshotV1 && msg.type === 'op' && this.log.currentSeq === msg.sequenceNumber) {
                this.engine.catchUps[this.doc].add(msg, this.log, lo, !!own);
            }
        });
        this.currentSeq = this.log.currentSeq;
    }
    updateSeqNumbers(min, seq) {
        this._queue(() => this.log.seqUpdate(min, seq));
        this.currentSeq = seq;
    }
    insertTextLocal(pos, text, props) {
        this._queue(() => { this.log.localInsert(pos, props ? { text, props } : text, this.engine.interner); this._countLocal(); });
    }
    insertMarkerLocal(pos, refType, props) {
        this._queue(() => {
            this.log.localInsert(pos, props ? { marker: { refType }, props } : { marker: { refType } }, this.engine.interner);
            this._countLocal();
        });
    }
    removeRangeLocal(start, end) { this._queue(() => { this.log.localRemove(start, end); this._countLocal(); }); }
    _countLocal() { if (this.log.collaborating) this.localSeq++; }  // a pending local op takes a localSeq
    /** Client.localTransaction (client.ts:1029-1048): every member op as a local (pending) op. */
    /**
     * Client.applyStashedOp(op) (client.ts:830-856): a stashed op of this client applied as a local op (GROUP: each
     * member); returns the local op metadata (one token per member: its pending SegmentGroup, which
     * regeneratePendingOp takes from the head of the pending queue).
     */
    applyStashedOp(op) {
        if (op.type === 3) return op.ops.map((o) => this.applyStashedOp(o));
        if (!this.log.collaborating) throw new Error('0x2db');  // "Applying op must generate a pending segment"
        this._queue(() => { this.log.localOp(op, this.engine.interner); this._countLocal(); });
        this.nStashed = (this.nStashed || 0) + 1;
        return { stashed: this.nStashed, type: op.type };
    }
    localTransaction(groupOp) {
        this._queue(() => { for (const op of groupOp.ops) { this.log.localOp(op, this.engine.interner); this._countLocal(); } });
    }
    annotateRangeLocal(start, end, props, combiningOp) {  // client.ts:245-260
        this._queue(() => { this.log.localAnnotate(start, end, props, this.engine.interner, combiningOp); this._countLocal(); });
    }
    /** Client.rollback(op, localOpMetadata) (client.ts:421-423) of the newest pending local op `op`. */
    rollback(op) { this._queue(() => this.log.rollback(op, this.engine.interner)); }
    /**
     * Client.regeneratePendingOp(resetOp, segmentGroup) (client.ts:917-960) for the oldest pending op
     * (`resetOp`, the op that was submitted): flushes the engine and returns the op to resubmit.
     */
    regeneratePendingOp(resetOp) {
        if (this.log.intervals !== undefined && this.log.currentSeq !== this.lastNormalization) {
            // client.ts:921-926: the "normalize" event (the interval collections rebase their pending ops) comes first
            for (const c of this.log.intervals.data.values()) this.log._intervals(() => c.onNormalize(this));
        }
        this.lastNormalization = this.log.currentSeq;
        let first = 0;
        this._queue(() => { first = this.log.regenerate(resetOp); });
        this.engine.flush();
        this._check();
        const recs = regenRecords(native().getDeltas(this.engine.h, this.doc));
        return regeneratedOp(resetOp, recs, first, (ref) => this._props(ref));
    }
    _props(ref) {  // a property set of this document's arena -> the properties object
        const w = native().getProps(this.engine.h, this.doc, ref);
        const it = this.engine.interner;
        const names = Array.from(it.keys.keys());  // ids are insertion order
        const out = {};
        for (let k = 0; k < w[0]; k++) out[names[w[1 + 2 * k]]] = JSON.parse(it.valBytes[w[2 + 2 * k]].toString('utf8'));
        return out;
    }
    /**
     * createPositionReference (sequence/src/intervalCollection.ts:697-724): a local reference at pos of the view
     * sequenceArgs = {referenceSequenceNumber, clientId} (default: this client's local view), slid off a
     * removed-and-acked segment when `slide` (Client.getSlideToSegment, client.ts:1085-1099), then
     * createLocalReferencePosition (client.ts:377-389).  -> a reference handle for the calls below.
     */
    createPositionReference(pos, refType, sequenceArgs, slide) {
        let id = 0;
        this._queue(() => { id = this.log.createRef(pos, refType, sequenceArgs, !!slide); });
        return { id, refType, client: this };
    }
    /**
     * Client.createLocalReferencePosition(segment, offset, refType) (client.ts:377-389) for a segment this
     * client's getContainingSegment returned, before any later edit: the same view and position.
     */
    createLocalReferencePosition(segment, offset, refType) {
        if (!segment || segment._at === undefined || segment._at.stamp !== this.log.nPushed) {
            throw new UnsupportedError('createLocalReferencePosition on a segment from before the last edit');
        }
        return this.createPositionReference(segment._at.start + (offset || 0), refType, segment._at.view, false);
    }
    /** Client.removeLocalReferencePosition (client.ts:394-396). */
    removeLocalReferencePosition(lref) { this._queue(() => this.log.removeRef(lref.id)); return lref; }
    /** Client.localReferencePositionToPosition (client.ts:398-403), on the device. */
    localReferencePositionToPosition(lref) {
        this.engine.flush();
        this._check();
        const p = native().getRefPositions(this.engine.h, this.doc);
        return lref.id < p.length ? p[lref.id] : DetachedReferencePosition;
    }
    /** LocalReference.getOffset (localReference.ts:110) and its segment's leaf index (-1: none / gone). */
    localReferenceSegment(lref) {
        this.engine.flush();
        this._check();
        const r = native().getRefInfo(this.engine.h, this.doc, lref.id);
        return { leafIndex: r[0], offset: r[1], held: r[3] === 1 };
    }
    getCurrentSeq() { return this.currentSeq; }
    // ---- interval collections (sequence/src/intervalCollection.ts; SharedSegmentSequence, sequence.ts:445-801)
    /** DefaultMap.populate of the SharedString summary's `header` blob, before load(). */
    loadIntervals(header) {
        this._queue(() => {
            this.log.intervals = new IntervalCollections();
            this.log._intervals(() => this.log.intervals.populate(header));
        });
    }
    /** loadFinished (sequence.ts:750-801): after load() and its catch-up messages, the collections attach. */
    loadFinished() {
        if (this.log.intervals !== undefined) this._queue(() => this.log._intervals(() => this.log.intervals.attach(this.log)));
    }
    /** getIntervalCollection(label) (sequence.ts:445-447): add(start, end, intervalType, props) on a string
     * that is not collaborating yet (a detached SharedString); remote ops arrive through applyMsg. */
    getIntervalCollection(label, emitter) {
        if (this.log.intervals === undefined) this.log.intervals = new IntervalCollections();
        const c = this.log.intervals.get(label);
        if (!this.log.collaborating) {
            return { add: (start, end, intervalType, props) => {
                this._queue(() => this.log._intervals(() => c.add(this.log, start, end, intervalType, props)));
            } };
        }
        // a collaborating client: IntervalCollection's API (intervalCollection.ts:1620-2338); emitter(opName, value,
        // localOpMetadata) receives each op to submit
        if (emitter) this.emitters.set(label, emitter);
        this.log.intervals.live = true;
        const run = (fn) => { const r = this.log._intervals(fn); this.engine.dirty = true; return r; };
        const self = this;
        // helpers.create("transient", ...): two Transient references at the local view; their compare keys are read
        // with the document's (one sync), then the ids go back to the free list -- a Transient reference is held by no
        // segment's collection (localReference.ts:260-298), so queries take no reference slot
        const transientKeys = (ranges) => {
            const ids = ranges.map(([a, b]) => [self.log.createRef(a, 0x100, undefined, false),
                self.log.createRef(b, 0x100, undefined, false)]);
            self.engine.dirty = true;
            const keys = self.refKeys();
            const out = self.log._intervals(() => ids.map(([ts, te]) => [refKey(keys, ts), refKey(keys, te)]));
            for (let k = ids.length - 1; k >= 0; k--) {
                self.log.releaseRef(ids[k][1], false);
                self.log.releaseRef(ids[k][0], false);
            }
            return [keys, out];
        };
        // the end tree (compareSequenceIntervalEnds, :1168-1169): one node per end; two intervals with equal ends
        // share a node that holds the later-put one -- a history this host does not keep, so it refuses
        const byEnd = (keys) => {
            const ivs = [...c.byId.values()].map((iv) => [refKey(keys, iv.end), iv]).sort((x, y) => cmpKey(x[0], y[0]));
            for (let k = 1; k < ivs.length; k++) {
                if (cmpKey(ivs[k - 1][0], ivs[k][0]) === 0) throw new IntervalUnsupported('two intervals with one end: the end tree keeps one node for them');
            }
            return ivs;
        };
        return {
            add: (start, end, intervalType, props) => run(() => c.liveAdd(self, start, end, intervalType, props)),
            change: (id, start, end) => run(() => c.liveChange(self, id, start, end)),
            changeProperties: (id, props) => run(() => c.liveChangeProperties(self, id, props)),
            removeIntervalById: (id) => run(() => c.liveRemove(self, id)),
            getIntervalById: (id) => c.byId.get(id),
            /** [start, end] positions (localReferencePositionToPosition of the endpoints) */
            positions(iv, keys) { const k = keys || self.refKeys(); return [k[4 * iv.start], k[4 * iv.end]]; },
            [Symbol.iterator]() { return self.log._intervals(() => c.ordered(self.refKeys()))[Symbol.iterator](); },
            findOverlappingIntervals(start, end) {  // :950-964 (SequenceInterval.overlaps in tree order)
                return this.findOverlappingIntervalsMany([[start, end]])[0];
            },
            /** findOverlappingIntervals for each [start, end] of `ranges`, from one engine sync */
            findOverlappingIntervalsMany(ranges) {
                const live = ranges.map((r, k) => k).filter((k) => ranges[k][1] >= ranges[k][0] && c.byId.size > 0);
                const out = ranges.map(() => []);
                if (live.length === 0) return out;
                const [keys, tk] = transientKeys(live.map((k) => ranges[k]));
                return self.log._intervals(() => {
                    const ordered = c.ordered(keys);
                    live.forEach((k, q) => {
                        const [ks, ke] = tk[q];
                        out[k] = ordered.filter((iv) => cmpKey(refKey(keys, iv.start), ke) <= 0 && cmpKey(refKey(keys, iv.end), ks) >= 0);
                    });
                    return out;
                });
            },
            previousInterval(pos) {  // :966-978: endIntervalTree.floor of a transient (pos, pos)
                const [keys, tk] = transientKeys([[pos, pos]]);
                return self.log._intervals(() => {
                    const k = tk[0][1];
                    let best;
                    for (const [e, iv] of byEnd(keys)) if (cmpKey(e, k) <= 0) best = iv;
                    return best;
                });
            },
            nextInterval(pos) {  // :980-992: endIntervalTree.ceil of a transient (pos, pos)
                const [keys, tk] = transientKeys([[pos, pos]]);
                return self.log._intervals(() => {
                    const k = tk[0][1];
                    for (const [e, iv] of byEnd(keys)) if (cmpKey(e, k) >= 0) return iv;
                    return undefined;
                });
            },
            // the positional iterators (:2232-2331, gatherIterationResults :864-944): the intervals whose start (and
            // end) compare equal to a transient interval's, forward or backward in the tree's order
            gather(forward = true, start, end) {
                if (start === undefined && end === undefined) {
                    const out = self.log._intervals(() => c.ordered(self.refKeys()));
                    return forward ? out : out.reverse();
                }
                const [keys, tk] = transientKeys([[start !== undefined ? start : 0, end !== undefined ? end : 0]]);
                const [ks, ke] = tk[0];
                let out = self.log._intervals(() => c.ordered(keys));
                if (start === undefined) out = out.filter((iv) => cmpKey(refKey(keys, iv.end), ke) === 0);
                else if (end === undefined) out = out.filter((iv) => cmpKey(refKey(keys, iv.start), ks) === 0);
                else out = out.filter((iv) => cmpKey(refKey(keys, iv.start), ks) === 0 && cmpKey(refKey(keys, iv.end), ke) === 0);
                return forward ? out : out.reverse();
            },
            // the same three queries from the device's read-only call (Collection.findOverlappingIntervals /
            // previousInterval / nextInterval over mtr_query_intervals): no Transient record, no reference slot;
            // previous / next refuse only when the answer's own end is shared, not whenever any two ends are
            device: {
                findOverlappingIntervals: (start, end) => self.log._intervals(() => c.findOverlappingIntervals(self, start, end)),
                findOverlappingIntervalsMany: (ranges) => self.log._intervals(() => c.findOverlappingIntervalsMany(self, ranges)),
                previousInterval: (pos) => self.log._intervals(() => c.previousInterval(self, pos)),
                nextInterval: (pos) => self.log._intervals(() => c.nextInterval(self, pos)),
            },
            CreateForwardIteratorWithStartPosition(pos) { return this.gather(true, pos, undefined)[Symbol.iterator](); },
            CreateBackwardIteratorWithStartPosition(pos) { return this.gather(false, pos, undefined)[Symbol.iterator](); },
            CreateForwardIteratorWithEndPosition(pos) { return this.gather(true, undefined, pos)[Symbol.iterator](); },
            CreateBackwardIteratorWithEndPosition(pos) { return this.gather(false, undefined, pos)[Symbol.iterator](); },
        };
    }
    /** The summary's `header` blob (summarizeCore, sequence.ts:467-480), undefined when there are no collections. */
    summarizeIntervals() {
        if (this.log.intervals === undefined) return undefined;
        this.engine.flush();
        this._check();
        const st = native().getRefStates(this.engine.h, this.doc);
        return this.log._intervals(() => this.log.intervals.serialize(st, this.log.currentSeq));
    }
    getText(start, end) {
        if (start !== undefined || end !== undefined) {  // SharedString.getText(start, end): a range of the local view
            return this.engine.getTextRanges([{ client: this, start, end }])[0];
        }
        this.engine.flush();
        this._check();
        return native().getText(this.engine.h, this.doc);
    }
    /** getLength: the local view's length (root.cachedLength; a marker counts 1). */
    getLength() {
        this.engine.flush();
        this._check();
        const me = this.log.collaborating ? this.log.clientIx.get(this.log.observerId) : -1;
        return native().getViewLength(this.engine.h, this.doc, this.log.currentSeq, me);
    }
    // ---- a live client's interval collections (what IntervalCollection needs from its Client and emitter)
    refKeys() { this.engine.flush(); this._check(); return native().getRefKeys(this.engine.h, this.doc); }
    /** BatchReplayEngine.queryIntervals over sets of this client's document (their doc is filled in) */
    queryIntervals(sets, refs, queries) {
        this.engine.flush();
        this._check();
        return this.engine.queryIntervals(sets.map((s) => ({ doc: this.doc, first: s.first, count: s.count })), refs, queries);
    }
    rebaseResults() {  // {record index -> position} of the MTR_OP_REBASE_POS records just queued
        this.engine.flush();
        this._check();
        const d = native().getDeltas(this.engine.h, this.doc);
        const out = new Map();
        for (let i = 0; i < d.length; i += 4) if (d[i + 3] === DELTA_REBASE) out.set(d[i], d[i + 1]);
        return out;
    }
    nextLocalSeq() {  // IntervalCollection.getNextLocalSeq (intervalCollection.ts:1584-1590)
        this._queue(() => this.log.bumpLocalSeq());
        return ++this.localSeq;
    }
    emit(label, opName, value, localOpMetadata) {  // the collection's IValueOpEmitter: an "act" op to submit
        const em = this.emitters.get(label);
        if (em) em(opName, value, localOpMetadata);
    }
    /**
     * SharedSegmentSequence.processCore's interval branch (sequence.ts:636-645) for a live client: `local` with the
     * op's localOpMetadata for this client's own ops (their acks).
     */
    processIntervalOp(msg, local, localOpMetadata) {
        let contents = msg.contents;
        if (typeof contents === 'string') contents = JSON.parse(contents);
        if (this.log.intervals === undefined) this.log.intervals = new IntervalCollections();
        this.engine._assertIdle();
        this.log._intervals(() => this.log.intervals.liveProcess(this, contents, msg, local, localOpMetadata));
        this.engine.dirty = true;
    }
    /** DefaultMap's resubmit of an interval op (rebaseLocalInterval, intervalCollection.ts:1270-1279) -> the op to send. */
    rebaseIntervalOp(contents, localOpMetadata) {
        const c = this.log.intervals.get(contents.key);
        const v = contents.value;
        const rebased = this.log._intervals(() => c.rebaseLocal(this, v.opName, v.value, localOpMetadata.localSeq));
        this.engine.dirty = true;
        return Object.assign({}, contents, { value: { opName: v.opName, value: rebased } });
    }
    /**
     * Client.getContainingSegment(pos, sequenceArgs) (client.ts:1065-1078): the segment holding pos in
     * the view of sequenceArgs = {referenceSequenceNumber, clientId} (default: this client's current
     * view), found on the device.  -> {segment: {text | marker, cachedLength, seq, clientId, removedSeq,
     * properties index}, offset} with both undefined when no segment covers pos.
     */
    getContainingSegment(pos, sequenceArgs) {
        this.engine.flush();
        this._check();
        const [ref, client] = this._viewOf(sequenceArgs);
        return this._containing(native().getContainingSegment(this.engine.h, this.doc, pos, ref, client), sequenceArgs);
    }
    /**
     * Client.resolveRemoteClientPosition(remotePos, remoteRefSeq, remoteClientId): the position in this client's
     * current view of what remotePos names in the remote client's view, undefined when that view holds no such
     * position.  (Many at once: BatchReplayEngine.resolveRemoteClientPositions.)
     */
    resolveRemoteClientPosition(pos, refSeq, clientId) {
        return this.engine.resolveRemoteClientPositions(
            [{ client: this, pos, sequenceArgs: { referenceSequenceNumber: refSeq, clientId } }])[0];
    }
    /**
     * Client.getPosition(segment) in this client's current view, the segment named by its tree-order ordinal
     * (getContainingSegment's segment.leafIndex); `offset` units are added, as resolveRemoteClientPosition adds them.
     * undefined for an ordinal the document does not hold.
     */
    getPosition({ leaf, offset }) {
        this.engine.flush();
        this._check();
        const [ref, client] = this._viewOf(undefined);
        const res = this.engine._transform([[this.doc, leaf, 0, 0, ref, client, POS_FROM_LEAF, offset === undefined ? 0 : offset]]);
        return res[0] < 0 ? undefined : res[0];
    }
    /**
     * SharedString.findTile(pos, label, preceding) in this client's current view: {pos, leaf, refType, props, seq} of
     * the nearest marker at or before (preceding, the default) or at or after pos whose referenceTileLabels hold the
     * label, undefined when there is none.  (Many at once: BatchReplayEngine.findTiles.)
     */
    findTile(pos, label, preceding = true) {
        return this.engine.findTiles([{ client: this, pos, label, preceding }])[0];
    }
    /**
     * SharedString.getMarkerFromId(id) with getPosition in this client's current view: {pos, leaf, refType, props, seq},
     * undefined for an id no marker has (or whose marker zamboni took out of the tree).  An id that block updates may
     * have remapped is refused, as a relative position on it is.
     */
    getMarkerFromId(id) {
        this.engine.flush();
        this._check();
        const k = id ? DocLog._idKey(id) : null;
        if (k === null || !this.log.markerIds.has(k)) return undefined;
        if (this.log.markerDup.has(k) || this.log.markerIdAnnotated) {
            throw new UnsupportedError('a marker id remapped by block updates');
        }
        const [ref, client] = this._viewOf(undefined);
        const q = new Int32Array([this.doc, this.log.markerIds.get(k), ref, client, MK_BY_ID, 0]);
        const res = native().findMarkers(this.engine.h, new ArrayBuffer(0), new ArrayBuffer(0), q.buffer);
        return BatchReplayEngine._markerHits(res, 1)[0];
    }
    /** sequenceArgs -> [refSeq, short client id] of the view (default: this client's current view). */
    _viewOf(sequenceArgs) {
        if (sequenceArgs === undefined) {  // getClientSequenceArgsForMessage, client.ts:598-630
            return [this.currentSeq, this.log.collaborating ? this.log.clientIx.get(this.log.observerId) : -1];
        }
        const cid = sequenceArgs.clientId === null || sequenceArgs.clientId === undefined ? 'null'
            : String(sequenceArgs.clientId);
        return [sequenceArgs.referenceSequenceNumber, this.log.shortId(cid)];  // getOrAddShortClientId
    }
    /** The addon's answer r (null: no segment covers pos) as getContainingSegment reports it. */
    _containing(r, sequenceArgs) {
        if (r === null) return { segment: undefined, offset: undefined };
        const longId = (c) => (c >= 0 ? this.log.clients[c] : 'original');
        // (a pending local segment: seq / removedSeq = UnassignedSequenceNumber with its localSeq, as
        // mergeTree.ts:1397-1427 / 1955-2047 leave them)
        const segment = { cachedLength: r.length, seq: r.seq, clientId: longId(r.client), leafIndex: r.leaf,
            removedSeq: r.removed ? r.removedSeq : undefined, propertySet: r.props < 0 ? undefined : r.props };
        // (where createLocalReferencePosition finds it again while no edit intervened)
        Object.defineProperty(segment, '_at', { value: { start: r.start, view: sequenceArgs,
            stamp: this.log.nPushed }, enumerable: false });
        if (r.localSeq >= 0) segment.localSeq = r.localSeq;
        if (r.localRemovedSeq >= 0) segment.localRemovedSeq = r.localRemovedSeq;
        if (r.marker) segment.marker = { refType: r.refType };
        else segment.text = r.text;
        return { segment, offset: r.offset };
    }
    /**
     * Client.summarize (client.ts:966-1000) -> ISummaryTreeWithStats.  In the legacy format the
     * catch-up messages are the shim's own transformed list (CatchUpLog): the caller's list was built
     * without sequenceDelta events, so it is superseded.
     */
    summarize(runtime, handle, serializer, catchUpMsgs) {
        const dm = runtime.deltaManager;
        this.updateSeqNumbers(dm.minimumSequenceNumber, dm.lastSequenceNumber);
        const v1 = !!this.engine.options.snapshotV1;
        if (v1 && catchUpMsgs !== undefined && catchUpMsgs.length > 0) throw new Error('0x03f');
        this.engine.flush();
        this._check();
        if (!this.engine.summarized) { native().summarize(this.engine.h); this.engine.summarized = true; }
        return this._summaryTree(catchUpMsgs, dm, handle, serializer, v1);
    }
    /** summarize on a worker thread: resolves to the same ISummaryTreeWithStats. */
    async summarizeAsync(runtime, handle, serializer, catchUpMsgs) {
        const dm = runtime.deltaManager;
        this.updateSeqNumbers(dm.minimumSequenceNumber, dm.lastSequenceNumber);
        const v1 = !!this.engine.options.snapshotV1;
        if (v1 && catchUpMsgs !== undefined && catchUpMsgs.length > 0) throw new Error('0x03f');
        await this.engine.summarizeAllAsync();
        this._check();
        return this._summaryTree(catchUpMsgs, dm, handle, serializer, v1);
    }
    /**
     * The git blob id (40 hex digits: gitHashFile's result, what Fluid's git storage names a blob by) of every blob
     * summarize() returns, by blob name: header, body / body_0..., and the legacy format's catch-up blob when there
     * is one.  The engine's blobs are hashed on the device (mtr_summary_blob_ids); the catch-up blob is built here,
     * so it is hashed here.  Takes summarize()'s arguments and steps (flush, summarize if needed); without a
     * runtime it describes the last summarize() of this client.
     */
    summaryBlobIds(runtime, handle, serializer, catchUpMsgs) {
        const dm = runtime ? runtime.deltaManager : this._summaryDm;
        if (!dm) throw new Error('summaryBlobIds: pass the runtime, or call summarize() first');
        const v1 = !!this.engine.options.snapshotV1;
        if (runtime) {
            this.updateSeqNumbers(dm.minimumSequenceNumber, dm.lastSequenceNumber);
            if (v1 && catchUpMsgs !== undefined && catchUpMsgs.length > 0) throw new Error('0x03f');
        }
        this.engine.flush();
        this._check();
        if (!this.engine.summarized) { native().summarize(this.engine.h); this.engine.summarized = true; }
        const { blobs, ids } = native().getSummary(this.engine.h, this.doc, true);
        const names = v1 ? blobs.map((_, i) => (i === 0 ? 'header' : 'body_' + (i - 1))) : ['header', 'body'];
        const res = {};
        ids.forEach((id, i) => { res[names[i]] = id; });
        if (!v1) {
            const msgs = this.engine.catchUps[this.doc].forSummary(dm.minimumSequenceNumber);
            if (msgs !== undefined && msgs.length > 0) {
                const s = Buffer.from(serializer ? serializer.stringify(msgs, handle) : JSON.stringify(msgs), 'utf8');
                res[this.engine.options.catchUpBlobName || 'catchupOps'] = require('crypto').createHash('sha1')
                    .update('blob ' + s.length + '\0').update(s).digest('hex');
            }
        }
        return res;
    }
    /**
     * The git tree id of the tree summarize() returns: the engine's blobs by their device-made ids, and this client's
     * own host blob (the legacy format's catch-up blob, hashed here as summaryBlobIds() does) passed in as an extra
     * entry (mtr_summary_tree_ids).  Takes summaryBlobIds()'s arguments.
     */
    summaryTreeId(runtime, handle, serializer, catchUpMsgs) {
        const ids = this.summaryBlobIds(runtime, handle, serializer, catchUpMsgs);
        const name = this.engine.options.catchUpBlobName || 'catchupOps';
        const extras = !this.engine.options.snapshotV1 && ids[name] !== undefined ? [{ name, id: ids[name] }] : [];
        return native().summaryTreeIds(this.engine.h, this.doc, this.doc + 1, [extras])[0];
    }
    _summaryTree(catchUpMsgs, dm, handle, serializer, v1) {
        this._summaryDm = { minimumSequenceNumber: dm.minimumSequenceNumber, lastSequenceNumber: dm.lastSequenceNumber };
        const blobs = native().getSummary(this.engine.h, this.doc);
        if (!v1) catchUpMsgs = this.engine.catchUps[this.doc].forSummary(dm.minimumSequenceNumber);
        const names = v1 ? blobs.map((_, i) => (i === 0 ? 'header' : 'body_' + (i - 1))) : ['header', 'body'];
        const tree = {};
        let total = 0;
        blobs.forEach((b, i) => { tree[names[i]] = { type: SummaryType.Blob, content: b.toString('utf8') }; total += b.length; });
        if (!v1 && catchUpMsgs !== undefined && catchUpMsgs.length > 0) {  // snapshotlegacy.ts:174-179
            const s = serializer ? serializer.stringify(catchUpMsgs, handle) : JSON.stringify(catchUpMsgs);
            tree[this.engine.options.catchUpBlobName || 'catchupOps'] = { type: SummaryType.Blob, content: s };
            total += Buffer.byteLength(s, 'utf8');
        }
        return {
            stats: { treeNodeCount: 1, blobNodeCount: Object.keys(tree).length, handleNodeCount: 0,
                totalBlobSize: total, unreferencedBlobSize: 0 },
            summary: { type: SummaryType.Tree, tree },
        };
    }
}

/**
 * A SharedMatrix observer (matrix/src/matrix.ts:636-693, remote branch) on a pair of engine documents:
 * applyMsg queues vector / set-cell messages; summarizeVectors returns each PermutationVector's summary
 * (V1 segments blobs + handleTable, permutationvector.ts:310-325).  (Cell values are host-side state;
 * the Python mirror fluidframework_amd/cells.py builds the cells blob from the engine's cell records.)
 */
class BatchMatrixClient {
    constructor(engine, rowsDoc) { this.engine = engine; this.doc = rowsDoc; this.log = engine.logs[rowsDoc]; }
    startOrUpdateCollaboration(longClientId, minSeq, currentSeq) {
        this.engine._assertIdle();
        this.log.startCollab(longClientId, minSeq || 0, currentSeq || 0);
        this.engine.dirty = true;
    }
    applyMsg(msg) { this.engine._assertIdle(); this.log.message(msg, this.engine.interner); this.engine.dirty = true; }
    summarizeVectors() {
        this.engine.flush();
        for (const d of [this.doc, this.doc + 1]) {
            const st = native().docStatus(this.engine.h, d);
            if (st[0] !== STATUS.OK) throw new Error('engine status ' + st[0] + ' at op ' + st[1]);
        }
        if (!this.engine.summarized) { native().summarize(this.engine.h); this.engine.summarized = true; }
        const vec = (d) => native().getSummary(this.engine.h, d).map((b) => b.toString('utf8'));
        return { rows: vec(this.doc), cols: vec(this.doc + 1) };
    }
}

module.exports = { BatchReplayEngine, BatchReplayClient, BatchMatrixClient, Interner, DocLog, MatrixDocLog, matrixLogs,
    regenRecords, regeneratedOp,
    buildBatch, UnsupportedError, OP, F, SummaryType, native };
