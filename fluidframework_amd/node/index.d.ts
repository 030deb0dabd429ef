/*
 * TypeScript declarations of the Node host shim (index.js): the observer subset of
 * @fluidframework/merge-tree's Client (packages/dds/merge-tree/src/client.ts:98) backed by the
 * MI355X engine through the N-API addon (mtr_napi.node) and the C ABI (include/mtr.h).
 */
import type { ISequencedDocumentMessage } from "@fluidframework/protocol-definitions";
import type { ISummaryTreeWithStats } from "@fluidframework/runtime-definitions";

/** IMergeTreeOptions subset (mergeTree.ts:400-438) plus engine capacities. */
export interface BatchReplayOptions {
	newLengthCalc?: 0 | 1; // mergeTreeUseNewLengthCalculations
	snapshotV1?: 0 | 1; // newMergeTreeSnapshotFormat
	chunkSize?: number; // mergeTreeSnapshotChunkSize (default 10000)
	catchUpBlobName?: string; // legacy catch-up blob name (default "catchupOps")
	device?: number; // HIP device ordinal
	maxSegments?: number;
	heapEntries?: number;
	textUnits?: number;
	propWords?: number;
	removerCells?: number;
	opsPerLaunch?: number;
}

/** Thrown for inputs outside the observer path: keep this document on the TypeScript Client. */
export class UnsupportedError extends Error {
	readonly fallback: true;
}

/** The observer Clients of many documents on one GPU; messages are applied in batches. */
export interface RangeQuery {
	client: BatchReplayClient;
	start?: number;
	end?: number;
	sequenceArgs?: { referenceSequenceNumber: number; clientId: string };
}

export class BatchReplayEngine {
	constructor(maxDocs: number, options?: BatchReplayOptions);
	createClient(): BatchReplayClient;
	/** A SharedMatrix observer: its rows / cols PermutationVectors as two engine documents. */
	createMatrix(): BatchMatrixClient;
	/** Apply every queued message of every document (done implicitly before any read). */
	flush(): void;
	/** flush() on a libuv worker thread (napi_async_work); other calls on this engine throw until it settles. */
	flushAsync(): Promise<void>;
	/**
	 * The summarizer's hand-over in one call (mtr_replay_pipelined): apply every queued message, build every
	 * document's summary and download the records -- document d's is bytes[docOff[d], docOff[d + 1]): u32 blob
	 * count, u32 blob lengths, the blobs (the same bytes summarize() returns as blob contents).  Batches of remote
	 * messages go through the pipelined path in `parts` document ranges (pipelined: true); others take the serial
	 * calls.  The per-client summarize() reads stay valid afterwards.
	 */
	replaySummaries(parts?: number): { bytes: Buffer; docOff: Float64Array; pipelined: boolean };
	/**
	 * replaySummaries that downloads only the blobs storage lacks (mtr_replay_handover): apply every queued message,
	 * build every document's summary, and sort every blob against the blob-id cache as summaryNovel() does -- document
	 * d's blobs are blobs[docFirst[d] .. docFirst[d + 1]), and only state-1 blobs carry bytes.  Batches of remote
	 * messages go through the pipelined path in `parts` document ranges (pipelined: true); others take the serial
	 * calls, with the same result.  summaryTreeIds() and blobCacheAddSummary() follow without hashing again.
	 */
	replayHandover(parts?: number): {
		blobs: { id: string; state: 0 | 1 | 2; rep: number; bytes?: Buffer }[];
		docFirst: number[];
		pipelined: boolean;
	};
	/**
	 * The incremental hand-over: the git blob ids of the current summary (flushed and summarized if needed) become
	 * the baseline, keyed by (document, blob index).  Call it once storage has acknowledged the upload.
	 */
	markSummaryBaseline(): void;
	/** Drop the baseline: every blob counts as changed. */
	clearSummaryBaseline(): void;
	/**
	 * Every blob of documents [lo, hi) in record order: ids[k] its git blob id, changed[k] its bytes when it is new
	 * or differs from the baseline and null when the baseline holds the same id at the same (document, index);
	 * document lo + i's blobs are [docFirst[i], docFirst[i + 1]).  Gathered on the device, one download
	 * (mtr_summary_delta).
	 */
	summaryDelta(lo?: number, hi?: number): { ids: string[]; changed: (Buffer | null)[]; docFirst: number[] };
	/**
	 * The blob-id cache: the set of git blob ids storage holds, under any path of any document, kept on the device
	 * (the stand-in for SummaryTreeUploadManager's blobsShaCache).  ids: 40-digit hex strings, or a Buffer of 20-byte
	 * ids.  It stays across batches, summaries and resets until blobCacheClear().
	 */
	blobCacheAdd(ids: string[] | Buffer): void;
	/** The ids of the current summary join the cache: call it once storage has acknowledged the upload. */
	blobCacheAddSummary(): void;
	blobCacheClear(): void;
	/** The number of distinct ids held. */
	blobCacheSize(): number;
	/** Per id: does the cache hold it (for the blobs the host makes itself). */
	blobCacheHas(ids: string[] | Buffer): boolean[];
	/**
	 * The cache's life cycle: every entry carries the generation at which its id was last offered (blobCacheAdd: the
	 * current one; blobCacheAddSummary moves to the next generation first).  The current generation.
	 */
	blobCacheGeneration(): number;
	/** ages[a] = the entries last referenced a generations ago, ages[n - 1] = all older ones; 1 <= n <= 1024. */
	blobCacheAges(n: number): number[];
	/** Drops the entries not referenced since minGeneration, on the device; returns how many. */
	blobCacheTrim(minGeneration: number): number;
	/** Trims to at most maxEntries entries by whole generations, oldest first; returns the entries removed. */
	blobCacheTrimTo(maxEntries: number): number;
	/** The entries in table order: 20-byte ids back to back, and their ages. */
	blobCacheExport(): { ids: Buffer; ages: number[] };
	/** Offers ids with their ages; importing an export into a fresh engine reproduces the cache. */
	blobCacheImport(ids: string[] | Buffer, ages: number[] | Uint32Array): void;
	/**
	 * Every blob of documents [lo, hi) in record order against the cache: state 0 the cache holds the id; 1 it is new
	 * and the first blob of the whole summary with that id (bytes holds it: upload it); 2 it is new but blob `rep` of
	 * this summary is the same object.  rep: a summary-wide blob index, the blob's own for state 1, -1 for state 0.
	 * Gathered on the device, one download (mtr_summary_novel).
	 */
	summaryNovel(lo?: number, hi?: number): { id: string; state: 0 | 1 | 2; rep: number; bytes?: Buffer }[];
	/**
	 * BatchReplayClient.getContainingSegment for many views of many documents in one batched call on the device
	 * (mtr_get_containing_segments); one result per query, in order.
	 */
	getContainingSegments(
		queries: {
			client: BatchReplayClient;
			pos: number;
			sequenceArgs?: { referenceSequenceNumber: number; clientId: string };
		}[],
	): ContainingSegment[];
	/**
	 * BatchReplayClient.resolveRemoteClientPosition for many positions of many documents in one batched call on the
	 * device (mtr_transform_positions): pos is a position of the sequenceArgs view; the answer is the position in that
	 * client's own current view, undefined where the reference returns undefined.  One result per query, in order.
	 */
	resolveRemoteClientPositions(
		queries: {
			client: BatchReplayClient;
			pos: number;
			sequenceArgs: { referenceSequenceNumber: number; clientId: string };
		}[],
	): (number | undefined)[];
	/**
	 * SharedString.findTile(pos, label, preceding) for many positions of many documents in one read-only batched call on
	 * the device (mtr_find_markers): the nearest marker at or before (preceding, the default) or at or after pos whose
	 * referenceTileLabels hold the label, at the (refSeq, clientId) view (default: that client's own current view);
	 * undefined where there is none.  One result per query, in order.
	 */
	findTiles(
		queries: {
			client: BatchReplayClient;
			pos: number;
			refSeq?: number;
			clientId?: string;
			label: string;
			preceding?: boolean;
		}[],
	): (MarkerHit | undefined)[];
	/**
	 * Interval queries over many collections of many documents in one read-only batched call on the device
	 * (mtr_query_intervals); mode 0 overlap, 1 previous, 2 next.  A hit is 8 int32 words: interval, startPos, endPos,
	 * startKey, startOff, endKey, endOff, flags (1: several intervals share that end); status 1: an endpoint of the set
	 * sits on a segment zamboni took out of the tree.
	 */
	queryIntervals(
		sets: { doc: number; first: number; count: number }[],
		refs: [number, number][],
		queries: { set: number; start: number; end?: number; mode: 0 | 1 | 2 }[],
	): { hitFirst: Float64Array; status: Int32Array; hits: Int32Array };
	/**
	 * The local references of many clients' documents in one batched call on the device (mtr_get_refs).  mode: the
	 * words per reference (1 positions, 2 positions and state bits, 4 the compare keys too); client i's words are
	 * words[mode * docFirst[i] .. mode * docFirst[i + 1]).
	 */
	getRefsBatch(clients: BatchReplayClient[], mode: 1 | 2 | 4): { docFirst: Float64Array; words: Int32Array };
	/**
	 * The delta records of many clients' documents in one batched call on the device (mtr_get_deltas_batch): client
	 * i's [op, pos, len, kind] records are records[4 * docFirst[i] .. 4 * docFirst[i + 1]).  With wantProps, record
	 * r's property words ([n, key id, value id, ...] for a regenerated insert's MTR_DELTA_REGEN_X record of a
	 * SharedString, none otherwise) are props[propsOff[r] .. propsOff[r + 1]).  The addon's own entry is
	 * getDeltasBatch(h, docs | null, n, wantProps), docs a Uint32Array of document indices, null = 0 .. n - 1.
	 */
	getDeltasBatch(
		clients: BatchReplayClient[],
		wantProps?: boolean,
	): { docFirst: Float64Array; records: Int32Array; propsOff?: Float64Array; props?: Uint32Array };
	/**
	 * Client.walkSegments(handler, start, end) for many ranges of many documents in one batched call on the device
	 * (mtr_get_range_segments): per query its segments in order, as getContainingSegment reports them; the first one's
	 * offset is the clip at start, a text segment's text holds its units inside the range.  start defaults to 0, end to
	 * the view's end; placeholder: one character a marker's text is.
	 */
	getRangeSegments(queries: RangeQuery[], placeholder?: string): ContainingSegment[][];
	/** getText(refSeq, clientId, placeholder, start, end) for many ranges in one batched call: text only, no segments */
	getTextRanges(queries: RangeQuery[], placeholder?: string): string[];
	/** git tree id of each document's summary tree; extras[i]: host-made entries of document lo + i's tree */
	summaryTreeIds(lo?: number, hi?: number, extras?: ({ name: string; id: string; tree?: boolean }[] | undefined)[]): string[];
}

/** getContainingSegment's answer (client.ts:1065-1078); both fields undefined when no segment covers pos. */
/** A marker found by findTiles / findTile / getMarkerFromId: its position in the view and mtr_segment_info's fields. */
export interface MarkerHit {
	pos: number;
	leaf: number;
	refType: number;
	/** the index of its property set (ContainingSegment.segment.propertySet), -1 when it has none */
	props: number;
	seq: number;
}

export interface ContainingSegment {
	segment?: {
		text?: string;
		marker?: { refType: number };
		cachedLength: number;
		seq: number;
		clientId: string; // the long id ("original" for the non-collaborating client)
		removedSeq?: number;
		leafIndex: number;
		propertySet?: number;
	};
	offset?: number;
}

/** SharedMatrix observer (matrix.ts:636-693, remote branch). */
export class BatchMatrixClient {
	startOrUpdateCollaboration(longClientId: string, minSeq?: number, currentSeq?: number): void;
	applyMsg(msg: ISequencedDocumentMessage): void;
	/** Each vector's PermutationVector.summarize blobs (V1 segments..., handleTable), permutationvector.ts:310-325. */
	summarizeVectors(): { rows: string[]; cols: string[] };
}

/** Drop-in for the observer use of `Client` (client.ts:98). */
export class BatchReplayClient {
	startOrUpdateCollaboration(longClientId: string, minSeq?: number, currentSeq?: number): void; // client.ts:1133
	applyMsg(msg: ISequencedDocumentMessage, local?: false): void; // client.ts:858
	updateSeqNumbers(min: number, seq: number): void; // client.ts:877
	insertTextLocal(pos: number, text: string, props?: Record<string, unknown>): void; // before collaboration only
	insertMarkerLocal(pos: number, refType: number, props?: Record<string, unknown>): void;
	removeRangeLocal(start: number, end: number): void;
	annotateRangeLocal(start: number, end: number, props: Record<string, unknown>): void;
	/** MergeTreeTextHelper.getText (MergeTreeTextHelper.ts:20-81): the local view's text, or its range [start, end) */
	getText(start?: number, end?: number): string;
	getLength(): number;
	getCurrentSeq(): number;
	/** interval collections (sequence/src/intervalCollection.ts): the summary's `header` blob before load ... */
	loadIntervals(header: string): void;
	/** ... and loadFinished (sequence.ts:750-801) after load and its catch-up messages */
	loadFinished(): void;
	/** a detached string's collection: add(start, end, intervalType, props with an intervalId) */
	getIntervalCollection(label: string): { add(start: number, end: number, intervalType: number, props: object): void };
	/** the summary's `header` blob (sequence.ts:467-480); undefined when there are no collections */
	summarizeIntervals(): string | undefined;
	summarize(
		runtime: { deltaManager: { minimumSequenceNumber: number; lastSequenceNumber: number } },
		handle: unknown,
		serializer: { stringify(value: unknown, bind: unknown): string } | undefined,
		catchUpMsgs: ISequencedDocumentMessage[],
	): ISummaryTreeWithStats; // client.ts:966
	/**
	 * Git blob id (40 hex digits, gitHashFile's result) of every blob of summarize(), by blob name: header, body /
	 * body_0..., the legacy catch-up blob when there is one.  The engine's blobs are hashed on the device.  Takes
	 * summarize()'s arguments and steps; without a runtime it describes this client's last summarize().
	 */
	summaryBlobIds(
		runtime?: { deltaManager: { minimumSequenceNumber: number; lastSequenceNumber: number } },
		handle?: unknown,
		serializer?: { stringify(value: unknown, bind: unknown): string },
		catchUpMsgs?: ISequencedDocumentMessage[],
	): Record<string, string>;
	/** git tree id of the tree summarize() returns (the catch-up blob passed to the engine as an extra entry) */
	summaryTreeId(
		runtime?: { deltaManager: { minimumSequenceNumber: number; lastSequenceNumber: number } },
		handle?: unknown,
		serializer?: { stringify(value: unknown, bind: unknown): string },
		catchUpMsgs?: ISequencedDocumentMessage[],
	): string;
	/** summarize with the GPU work on a worker thread. */
	summarizeAsync(
		runtime: { deltaManager: { minimumSequenceNumber: number; lastSequenceNumber: number } },
		handle: unknown,
		serializer: { stringify(value: unknown, bind: unknown): string } | undefined,
		catchUpMsgs: ISequencedDocumentMessage[],
	): Promise<ISummaryTreeWithStats>;
	/** client.ts:1065: the segment holding pos at sequenceArgs' view (default: this client's current view). */
	getContainingSegment(
		pos: number,
		sequenceArgs?: { referenceSequenceNumber: number; clientId: string },
	): ContainingSegment;
	/**
	 * Client.resolveRemoteClientPosition: the position in this client's current view of what remotePos names in the
	 * (remoteRefSeq, remoteClientId) view; undefined when that view holds no such position.
	 */
	resolveRemoteClientPosition(remotePos: number, remoteRefSeq: number, remoteClientId: string): number | undefined;
	/**
	 * Client.getPosition(segment) in this client's current view plus offset, the segment named by its tree-order
	 * ordinal (ContainingSegment.segment.leafIndex); undefined for an ordinal the document does not hold.
	 */
	getPosition(segment: { leaf: number; offset?: number }): number | undefined;
	/** SharedString.findTile in this client's current view (many at once: BatchReplayEngine.findTiles). */
	findTile(pos: number, label: string, preceding?: boolean): MarkerHit | undefined;
	/**
	 * SharedString.getMarkerFromId with getPosition in this client's current view; undefined for an id no marker has or
	 * whose marker left the tree.  Throws UnsupportedError for an id that block updates may have remapped.
	 */
	getMarkerFromId(id: string | number | boolean): MarkerHit | undefined;
}
