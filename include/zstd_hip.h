/* include/zstd_hip.h -- C ABI of libzstd_hip.so, the MI355X (gfx950) backend for python-zstandard's
 * batch / one-shot frame hot path.
 *
 * Plain C, plain pointers and sizes, no torch / Python types. These entry points are what the reference's
 * C extension would bind in place of its file-local batch workers:
 *
 *   zhip_compress_batch    replaces  compress_from_datasources()   c-ext/compressor.c:1083-1336
 *                                    + compress_worker()           c-ext/compressor.c:856-1076
 *   zhip_decompress_batch  replaces  decompress_from_framesources() c-ext/decompressor.c:1185-1455
 *                                    + decompress_worker()          c-ext/decompressor.c:944-1181
 *   zhip_item              ==        DataSource / FramePointer      c-ext/compressor.c:805-808, decompressor.c:892-896
 *   zhip_segment           ==        BufferSegment                  c-ext/python-zstandard.h:307-313
 *   zhip_outbuf            ==        CompressorDestBuffer / DecompressorDestBuffer (compressor.c:816-821,
 *                                    decompressor.c:904-909): malloc()ed by the callee, ownership passes to the
 *                                    caller exactly like BufferWithSegments_FromMemory(useFree=1) expects
 *                                    (c-ext/bufferutil.c:107-148).
 *   error classes          ==        CompressorWorkerError / DecompressorWorkerError (compressor.c:823-828,
 *                                    decompressor.c:911-917) + first failing item index + zstd error code
 *                                    (numeric values of zstd/zstd_errors.h:61-97).
 *
 * The *_device entry points are the same operations with every buffer already resident in HBM
 * (what bench.py times and what a multi-GPU caller shards); the host-buffer entry points wrap them with
 * H2D / D2H copies. INTEGRATION.md shows the reference-side stub.
 */
#ifndef ZSTD_HIP_H
#define ZSTD_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ZHIP_ABI_VERSION 3

typedef struct { uint64_t offset, length; } zhip_segment;             /* BufferSegment */
typedef struct { const void* src; size_t srcSize; size_t dstSize; } zhip_item; /* dstSize: decompress only (0 = unknown) */
typedef struct { void* data; size_t dataSize; zhip_segment* segs; size_t nSegs; } zhip_outbuf;

/* worker error classes (values follow the reference enums) */
enum {
    ZHIP_ERR_NONE = 0,
    ZHIP_ERR_ZSTD = 1,          /* zstdErr holds the zstd error code */
    ZHIP_ERR_NO_MEMORY = 2,
    ZHIP_ERR_SIZE_MISMATCH = 3, /* decompress: produced != expected (errDetail = produced, expected) ; compress: nospace */
    ZHIP_ERR_UNKNOWN_SIZE = 4,  /* decompress: frame has no content size and none supplied */
    ZHIP_ERR_HIP = 5,           /* HIP runtime failure; zhip_last_error() has the text */
    ZHIP_ERR_UNSUPPORTED = 6    /* parameter combination not implemented by this backend (fails loudly) */
};

typedef struct {
    int kind;            /* ZHIP_ERR_* */
    int zstdErr;         /* zstd error code when kind == ZHIP_ERR_ZSTD */
    size_t index;        /* first failing item */
    uint64_t detail[2];  /* size mismatch: produced, expected */
} zhip_error;

/* dictionary content type == ZSTD_dictContentType_e (zstd/zstd.h; ZstdCompressionDict(data, dict_type=...), c-ext/compressiondict.c:170-191,
 * consumed at c-ext/compressor.c:37-52 and c-ext/compressiondict.c:148-162): AUTO = a blob that starts with the dictionary magic is a
 * full dictionary, anything else raw content; RAWCONTENT = content whatever the first bytes are; FULLDICT = the magic is required
 * (compression reports "Dictionary mismatch", decompression "Dictionary is corrupted", as libzstd does). */
enum { ZHIP_DICT_AUTO = 0, ZHIP_DICT_RAWCONTENT = 1, ZHIP_DICT_FULLDICT = 2 };
/* frame format == ZSTD_format_e (ZstdCompressionParameters(format=...), ZstdDecompressor(format=...), c-ext/decompressor.c:32-35):
 * MAGICLESS frames have no 4-byte magic number in front of the frame header. */
enum { ZHIP_FORMAT_ZSTD1 = 0, ZHIP_FORMAT_ZSTD1_MAGICLESS = 1 };
/* explicit compression parameters == ZSTD_compressionParameters; the reference keeps them in the ZSTD_CCtx_params it applies to every
 * worker context (c-ext/compressor.c:20,203,1138; c-ext/compressionparams.c:13-120). 0 = "take it from the level" for each field,
 * exactly like ZSTD_CCtxParams_setParameter(…, 0). strategy: 1 = fast and 2 = dfast are the strategies this backend implements for every
 * source; 3 = greedy where libzstd runs it with its row match finder on 16-entry rows over one block -- sources of 16 385 ... 131 072 bytes
 * (what level 5 resolves to there), a window of 2^15 or more that covers the whole source (an explicit windowLog of 15 or 16 on a larger
 * source is refused, as for every strategy), searchLog <= 4, hashLog <= 17 after the windowLog + 1 cap, no dictionary. A combination that resolves to anything else fails
 * loudly: ZHIP_ERR_UNSUPPORTED from zhip_ctx_set_cparams where no source could be served, else status 40 for the frame. */
typedef struct { uint32_t windowLog, chainLog, hashLog, searchLog, minMatch, targetLength; int32_t strategy; } zhip_compression_parameters;

/* compression parameters the hot path reads (the reference keeps them in ZSTD_CCtx_params,
 * c-ext/compressor.c:209-233; defaults there: contentSize=1, checksum=0, dictID=1). */
typedef struct {
    int level;
    int contentSizeFlag, checksumFlag, dictIDFlag;
    const void* dict; size_t dictSize;      /* raw bytes of a ZstdCompressionDict (or NULL) */
    int dictType;                           /* ZHIP_DICT_* */
    int format;                             /* ZHIP_FORMAT_* */
    zhip_compression_parameters cp;         /* all zero = derive everything from `level` */
} zhip_cparams;

typedef struct {
    const void* dict; size_t dictSize;      /* raw bytes of a ZstdCompressionDict (or NULL) */
    uint64_t maxWindowSize;                 /* 0 = default (1 << 27) */
    int dictType;                           /* ZHIP_DICT_* */
    int format;                             /* ZHIP_FORMAT_* */
} zhip_dparams;

/* ---- library / device ---- */
int         zhip_abi_version(void);
int         zhip_device_count(void);
int         zhip_set_device(int device);
const char* zhip_last_error(void);                  /* thread-local text of the last ZHIP_ERR_HIP */
const char* zhip_error_name(int zstdErr);            /* same strings as ZSTD_getErrorName (zstd.c:3580-3616) */
int         zhip_selftest(void);                     /* 0 = the wave primitives behave on this GPU */
size_t      zhip_compress_bound(size_t srcSize);     /* ZSTD_compressBound, zstd.h:249 */

/* ---- frame inspection (host, no GPU): ZSTD_getFrameContentSize zstd.c:43790, ZSTD_findFrameCompressedSize :44022 */
#define ZHIP_CONTENTSIZE_UNKNOWN ((uint64_t)-1)
#define ZHIP_CONTENTSIZE_ERROR   ((uint64_t)-2)
uint64_t zhip_frame_content_size(const void* src, size_t srcSize);
int64_t  zhip_find_frame_compressed_size(const void* src, size_t srcSize);  /* <0: -(zstd error code) */
/* the same with an explicit frame format (ZSTD_getFrameHeader_advanced zstd.c:43668, ZSTD_findFrameCompressedSize_advanced) */
uint64_t zhip_frame_content_size_format(const void* src, size_t srcSize, int format);
int64_t  zhip_find_frame_compressed_size_format(const void* src, size_t srcSize, int format);
/* level + size hints -> the parameters libzstd would use (ZSTD_getCParams zstd.c:30863; ZstdCompressionParameters.from_level,
 * c-ext/compressionparams.c:231-345). Host only. */
void     zhip_get_cparams(int level, uint64_t srcSizeHint, size_t dictSize, zhip_compression_parameters* out);
/* bytes of device memory the calling thread's contexts hold (scratch arenas, tables, staging; they grow with the largest batch seen and
 * are trimmed after very large ones) -- what ZstdCompressor.memory_size() / ZstdDecompressor.memory_size() report here, where the
 * reference reports ZSTD_sizeof_CCtx / ZSTD_sizeof_DCtx (c-ext/compressor.c:263, c-ext/decompressor.c:128). Creates the thread's context
 * (and its launch counters) if it does not exist yet, as the reference's contexts exist from the constructor on; 0 without a GPU. */
size_t   zhip_thread_memory_size(void);

/* ---- host-buffer batch API (drop-in for the reference's workers) ----
 * items are borrowed; *out is an array of *nOut buffers the caller owns -- one per pipeline chunk, like the reference's one per worker
 * (CompressorDestBuffer / DecompressorDestBuffer): release each `data` with zhip_free_payload() (large payloads are PINNED host
 * memory from a process-wide pool, so that the D2H copy lands in them at link speed; free() is correct only for the `segs` arrays),
 * each `segs` with free(), then the array with free() -- or everything with zhip_free_outbufs(bufs, n, 1).
 * Returns ZHIP_ERR_NONE or fills *err. Re-entrant; call with the GIL released. */
int  zhip_compress_batch(const zhip_cparams* params, const zhip_item* items, size_t n,
                         zhip_outbuf** out, size_t* nOut, zhip_error* err);
int  zhip_decompress_batch(const zhip_dparams* params, const zhip_item* items, size_t n, int requireSizes,
                           zhip_outbuf** out, size_t* nOut, zhip_error* err);
/* One call, every device (round 6). Both calls fan the batch out over the node's GPUs INSIDE the call, the way the reference fans it out over its worker
 * threads (c-ext/compressor.c:1127-1298, c-ext/decompressor.c:1237-1455): the item list is cut into contiguous runs of (almost) equal input bytes --
 * zhip_partition_by_bytes, the reference's rule -- every run goes to a host thread bound to its device (one persistent thread, context and staging area per
 * device slot), and the devices' zhip_outbufs come back in device order, which is item order; the first failing item (lowest index) is the one reported.
 * No collective is involved: the collection simply holds the buffers of every device. The environment selects the device slots: ZHIP_DEVICES=0,1,... (a
 * device may be listed twice: two contexts on one GPU); unset = every visible device, but at least ZHIP_DEVICE_MIN_BYTES (default 256 MiB) of input per
 * device, so small batches run on the calling thread's current device as they always did. Nothing changes for a caller. */
size_t zhip_partition_by_bytes(const uint64_t* sizes, size_t n, size_t workers, size_t* bounds /* 2 * workers: [start, end) per worker */);
int    zhip_batch_devices(int* devices, int cap);   /* the device slots the two calls above fan out over; returns their number */
void zhip_free_outbufs(zhip_outbuf* bufs, size_t n, int freePayload);
void zhip_free_payload(void* data);     /* a zhip_outbuf.data pointer: back to the pinned pool, or free() */

/* ---- device-resident batch API (all pointers are HBM addresses on the current device) ----
 * A context owns the per-launch scratch (literal buffers, hash tables, work counters, status words) so repeated
 * calls allocate nothing. `stream` is a hipStream_t passed as void* (NULL = default stream). Calls are asynchronous;
 * zhip_ctx_sync() waits and returns the first failing frame (lowest index) like the reference's workers do.
 *
 * Ordering and threads (pinned by tests/test_gpu_streams.py and tests/test_gpu_concurrent_callers.py):
 *   Stream order.   zhip_decompress_batch_device, zhip_compress_batch_device and zhip_compact_device are ordered after everything queued on
 *                   `stream` before the call, and everything queued on `stream` after the call returns sees all of its outputs (d_dst,
 *                   d_outSizes, d_status): producers and consumers on the same stream need no host synchronisation, a blocking or a
 *                   non-blocking stream alike. The library's internal streams (the decode pipeline's chunk slots and their side streams) are
 *                   joined to `stream` at both ends of every call and never show to the caller. Work on OTHER streams is the caller's to order.
 *                   A call may wait on the host while it (re)allocates scratch or -- the first compress launch of 16 384 sources or more -- picks
 *                   its tables; it never needs the caller to.
 *   One call sequence per context.  A context is one queue of calls: calls on it may follow each other with nothing waited for in between
 *                   when they are made from one host thread at a time and on one stream (scratch is reused in stream order). Two host threads on
 *                   one context, or two streams on one context with work in flight on both, need the caller's own ordering. Different
 *                   contexts are independent: any threads, any streams.
 *   Setters.        zhip_ctx_set_ddict and zhip_ctx_set_cparams may be called between asynchronous calls without waiting for them: a setter that
 *                   uploads or digests anything (another dictionary, the same dictionary for other parameters) first waits for ALL work in
 *                   flight on the device, so calls queued before it finish with the tables they were queued with and calls made after it use
 *                   the new ones. A setter that finds its dictionary already digested (the fingerprint matches), clears the dictionary or
 *                   changes only level / flags / format / size hint touches host state, which every call reads when it is made, and does not wait.
 *   Host-buffer calls.  zhip_compress_batch / zhip_decompress_batch and zhip_thread_memory_size may be called from any number of threads
 *                   concurrently (contexts are per thread, the pinned pool and the device slots' worker threads are shared and serialise
 *                   inside); a payload may be released with zhip_free_payload / zhip_free_outbufs on any thread, also after the thread that
 *                   received it has exited. */
typedef struct zhip_ctx zhip_ctx;
zhip_ctx* zhip_ctx_create(void);
void      zhip_ctx_destroy(zhip_ctx*);
int       zhip_ctx_set_ddict(zhip_ctx*, const void* hostDict, size_t dictSize, int dictType);   /* parses + uploads; NULL clears */
int       zhip_ctx_set_dformat(zhip_ctx*, int format, uint64_t maxWindowSize);     /* frame format + window limit of the next decode calls */
int       zhip_ctx_set_cparams(zhip_ctx*, const zhip_cparams* params);            /* uploads dict / tables */
/* What a device-API caller knows about the UNCOMPRESSED size of its largest item (0 = nothing; the host-buffer API sees the sizes itself).
 * Items above one block (128 KiB) are frames of several blocks. Told so, decompression runs the phase-split kernels in their several-block
 * mode (a block is the work item) and compression gives the generic kernel the whole chip -- or, in batches of thousands of such sources, the
 * flat match kernel searches them too. Untold, they are decoded / encoded one wave per frame by a token grid of the generic kernels: correct,
 * slow (the reference has no equivalent: its workers take any size, c-ext/compressor.c:1035). Frames of ONE block's size may also be frames of several
 * blocks -- libzstd's block splitter (levels 16 and up) cuts a 128 KiB source into many --: a decompress caller whose frames come from such levels
 * should say 131 073 or more here (the host-buffer API counts every frame's blocks itself and does). */
void      zhip_ctx_set_size_hint(zhip_ctx*, uint64_t maxItemBytes);

/* d_src: concatenated frames; d_srcSegs[i] = (offset,length) of frame i in d_src.
 * d_dst: output arena;        d_dstSegs[i] = (offset, capacity) where frame i must be written.
 * d_outSizes[i] receives the produced size, d_status[i] 0 or a zstd error code. */
int zhip_decompress_batch_device(zhip_ctx*, const void* d_src, const zhip_segment* d_srcSegs, size_t n,
                                 void* d_dst, const zhip_segment* d_dstSegs,
                                 uint64_t* d_outSizes, int32_t* d_status, void* stream);
/* d_dstSegs[i].length must be >= zhip_compress_bound(d_srcSegs[i].length): every kernel that may serve an item (one-block sources, sources of
 * several blocks, any batch size) refuses a smaller slot with d_status[i] = 70 (Destination buffer is too small) and writes nothing into it,
 * however small the frame would have come out. Segments need no alignment and may come in any order; several items may name one source.
 * Nothing outside [offset, offset + length) of an item's destination segment is written, in either direction. */
int zhip_compress_batch_device(zhip_ctx*, const void* d_src, const zhip_segment* d_srcSegs, size_t n,
                               void* d_dst, const zhip_segment* d_dstSegs,
                               uint64_t* d_outSizes, int32_t* d_status, void* stream);
/* Compression from sequences the CALLER supplies: the match search of zhip_compress_batch_device is skipped, everything behind it -- entropy coding, block and
 * frame assembly, checksums -- is that call's, with the context's zhip_ctx_set_cparams state (level, parameters, frame flags, format, dictionary) and under the
 * same stream-order and one-call-sequence-per-context rules. For an external match finder (the frames are what ZSTD_compressSequences writes with explicit block
 * delimiters for the same list), and for tests that hand the entropy stage exact sequence lists. Sources of ONE block: at most 131 072 bytes (with a dictionary:
 * at most what the batch call's match kernels take); a larger source gets d_status 40 (Unsupported parameter).
 * d_seqs: packed sequences of the whole batch, 8 bytes each, little-endian fields
 *     bits  0..27  offBase      1, 2, 3 = repeat offset 1, 2, 3 (with litLength 0: 2, 3, and "repeat offset 1 minus one"); offset + 3 otherwise
 *     bits 28..45  litLength    literals copied in front of the match
 *     bits 46..63  matchLength  the match's full length, 3 or more
 * in source order; what the sequences of a source do not cover is its last literal run. d_seqSegs[i] = (first, count): source i's list is
 * d_seqs[first .. first + count). count 0 is a source without matches.
 * Checked per source, because the entropy stage relies on it: count <= the sequence capacity of a slot (43 704; fewer in a dictionary batch), every matchLength
 * >= 3, every offBase != 0, litLength + matchLength over the list sum to at most the source's size. A list that fails gets d_status 107 (External sequences are
 * not valid), size 0, nothing written to its destination; the other sources of the batch are unaffected. Offsets are NOT validated (as in libzstd with
 * ZSTD_c_validateSequences off): a list whose offsets do not reproduce the source yields a well-formed frame of other content. Whether a raw offset that equals a
 * repeat offset is coded as the repeat code is the caller's choice; libzstd writes the same bytes for the same codes.
 * flags: bit 0 clear = the entropy kernel gathers the literals from the source through the sequences (what the flat match kernels leave it); set = the loader
 * copies them to the context's literal area first (what the lane-serial match kernel leaves). The frames are the same. Other bits: ZHIP_ERR_UNSUPPORTED. */
int zhip_compress_sequences_device(zhip_ctx*, const void* d_src, const zhip_segment* d_srcSegs, size_t n,
                                   const uint64_t* d_seqs, const zhip_segment* d_seqSegs,
                                   void* d_dst, const zhip_segment* d_dstSegs,
                                   uint64_t* d_outSizes, int32_t* d_status, void* stream, uint32_t flags);
/* Which match finder zhip_compress_batch_device runs -- and with it zhip_seekable_compress_device and zhip_seekable_compress_records_device, which call it. Host state
 * only, never waits (the call itself does under ZHIP_FINDER_AUTO: below); the default is ZHIP_FINDER_LIBZSTD. Not read by zhip_compress_sequences_device or by the host-buffer API (zhip_compress_batch), whose contract is
 * libzstd's bytes.
 *   ZHIP_FINDER_LIBZSTD  the searches that keep libzstd's table contents: frames byte for byte libzstd's.
 *   ZHIP_FINDER_WAVE     one wave per source, a hash table of positions in LDS, 64 positions probed per trip (zhip_encode_wave.hpp), launched once per chunk in place of
 *                        every other match kernel. The frames are valid zstd that every zstd decoder reads; they are NOT libzstd's bytes: a different parse from a
 *                        4 096-cell table, measured 7-8 % larger than libzstd's at level 1 and 17-19 % larger at level 3 on 128 KiB sources, -1 % and +10 % on 4 KiB documents
 *                        (what it buys is time: 1.5-1.9 x at 16 384 x 128 KiB, 10 x and more on batches of a thousand sources and fewer).
 *                        They are deterministic: a pure function of the source and the context's parameters, the same on every run and device. (The ZHIP_WAVE_HLOG
 *                        environment variable, a measurement aid of tests/tools/wave_finder_rate.py, changes the table size and with it the bytes: a process that sets
 *                        it has given that up.)
 *                        The level still governs everything behind the search (table modes, raw literals at negative levels, frame flags, format, checksum).
 *                        Scope: sources of one block (<= 131 072 bytes), no dictionary, a level or parameters whose row for 16 385 ... 131 072-byte sources is fast or
 *                        double-fast (levels <= 4, negative levels, explicit strategy 1 / 2). A context with a dictionary, or outside those levels, makes the compress
 *                        call return ZHIP_ERR_UNSUPPORTED with a zhip_last_error() text that names the finder. A source of several blocks gets d_status 40 at its own
 *                        index and its neighbours compress; so does a source the row of its own size class does not serve (level 4 at 16 384 bytes and below, a window
 *                        that does not cover the source). Slot rules (zhip_compress_bound, d_status 70) are unchanged.
 *   ZHIP_FINDER_NONE     no match search at all, for NUMERIC TENSORS (float weights and activations, above all the byte planes of a typed seekable stream): one kernel
 *                        per chunk (zhip_encode_none.hpp) in place of the match kernels AND the entropy kernel, one wave per source, the source itself read as the block's
 *                        literals -- no sequence arena, no tables, no literal copy. Every frame is byte for byte what libzstd 1.5.7's ZSTD_compressSequences writes for
 *                        that source with explicit block delimiters and a list that is only the delimiter (litLength = the source's size) under the context's level,
 *                        parameters, frame flags and format -- which is also what zhip_compress_sequences_device writes for count 0: a literals section (Huffman, raw
 *                        or RLE) and "0 sequences", or a raw block where that gains less than ZSTD_minGain. The level still governs what it governs behind the search:
 *                        window descriptor, raw literals at negative levels (the whole block then comes out raw: allowed, and pointless), ZSTD_minGain, checksum,
 *                        content size, magicless format. On float tensors such frames are the size of level 3's or up to 13 % smaller (the search finds only short,
 *                        worthless matches there); on data with real repetition they lose badly -- 1.9 x level 3's size on int64 running sums, worse on text
 *                        (DESIGN.md 4.2 has the table). Pick it per context for data known to be numeric; nothing chooses it automatically.
 *                        Scope and refusals are the wave finder's: sources of one block (<= 131 072 bytes), no dictionary, a level or parameters whose row for
 *                        16 385 ... 131 072-byte sources is fast or double-fast (levels <= 4, negative levels, explicit strategy 1 / 2). A context with a dictionary,
 *                        or outside those levels, makes the compress call return ZHIP_ERR_UNSUPPORTED with a zhip_last_error() text that names the finder
 *                        ("ZHIP_FINDER_NONE", match finder "none"). A source of several blocks gets d_status 40 at its own index and its neighbours compress; so does
 *                        a source the row of its own size class does not serve (level 4 at 16 384 bytes and below, a window that does not cover the source). Slot
 *                        rules (zhip_compress_bound, d_status 70) are unchanged.
 *   ZHIP_FINDER_AUTO     ZHIP_FINDER_NONE or ZHIP_FINDER_LIBZSTD, chosen PER SOURCE: the right finder is a property of a frame, not of a tensor (of one int64 tensor's eight
 *                        byte planes some want the search by two orders of magnitude and some are smaller and 20-30 x cheaper without it). A classify kernel
 *                        (zhip_encode_auto.hpp, zhip_classify_batch_device below) reads a bounded sample of every source -- at most 14 KiB of a 128 KiB one -- and decides
 *                        from the sample's byte histogram and from what the matches it finds there would save over their bytes as literals; the batch is split in
 *                        device memory by that decision and the two parts run through the two finders' code as it is. Every frame is byte for byte what
 *                        ZHIP_FINDER_NONE or ZHIP_FINDER_LIBZSTD writes for that source -- libzstd's bytes for a well-defined libzstd call either way -- with d_status
 *                        and d_outSizes at the source's own index. The decision is a pure function of the source's bytes: not of the level, the batch, the launch
 *                        shape or the device. A source above one block or below 64 bytes goes to the search unsampled; a tie goes to the literals-only frame.
 *                        UNLIKE THE OTHER FINDERS THE CALL WAITS ONCE ON THE STREAM, for the two parts' sizes (8 bytes): the launch arguments of the existing kernels
 *                        carry their count by value. It is therefore not capturable into a graph. A part that is empty launches nothing.
 *                        Scope and refusals of the CALL are ZHIP_FINDER_NONE's (either part may be its kernel's): no dictionary, a level whose one-block row is fast or
 *                        double-fast, else ZHIP_ERR_UNSUPPORTED with a zhip_last_error() text that names the finder ("ZHIP_FINDER_AUTO", match finder "auto").
 *                        Per source they are the chosen finder's: a source of several blocks goes to the search, which serves it. DESIGN.md 4.2 has the rule, its
 *                        constants and what it costs against the better choice per frame.
 * An unknown value (3 among them): ZHIP_ERR_UNSUPPORTED, the finder stays what it was. */
enum { ZHIP_FINDER_LIBZSTD = 0, ZHIP_FINDER_WAVE = 1, ZHIP_FINDER_NONE = 2, ZHIP_FINDER_AUTO = 4 };
int zhip_ctx_set_match_finder(zhip_ctx*, int finder);
/* ZHIP_FINDER_AUTO's decision on its own, for a caller who routes frames itself: d_choice[i] = 0 (the search) or 1 (literals only) for source i of the batch, and, where
 * d_stats is not null, d_stats[4 i ...] = the integers it was made from -- sampled window bytes, their order-0 cost and the matches' credit in 1/256 bit, sampled positions
 * with a candidate of 4 bytes or more (all 0 for a source that was not sampled). Asynchronous and stream-ordered, no host wait except while scratch grows; reads the
 * sources only. A null d_choice or d_srcSegs: ZHIP_ERR_UNSUPPORTED, nothing queued. Does not read the context's level, finder or dictionary. */
int zhip_classify_batch_device(zhip_ctx*, const void* d_src, const zhip_segment* d_srcSegs, size_t n, uint8_t* d_choice, uint32_t* d_stats /* may be null */, void* stream);
size_t zhip_ctx_entropy_grid(zhip_ctx*);    /* waves of the entropy kernel resident on the context's device: a batch above it gives every wave several frames (for tests) */
int zhip_ctx_sync(zhip_ctx*, void* stream, const int32_t* d_status, size_t n, zhip_error* err);
/* The compress direction writes every frame into a zhip_compress_bound-sized slot; what is handed on (a BufferWithSegments, a payload
 * all-gatherv across GPUs) is the frames back to back. d_offsets[i] = where frame i goes inside d_dense (the caller's exclusive prefix
 * sum of d_outSizes, 8 bytes per item on the device); items whose d_status is non-zero are skipped. One wave per frame, 16 bytes per
 * lane. The collection step of c-ext/compressor.c:1407-1496 (per-worker destination buffers -> one result), on the device. */
int zhip_compact_device(const void* d_slots, const zhip_segment* d_slotSegs, const uint64_t* d_outSizes, const int32_t* d_status,
                        const uint64_t* d_offsets, size_t n, void* d_dense, void* stream);

/* ---- seekable streams: one large HBM buffer compressed as a batch, any byte range read back ----
 * The zstd seekable format: independent frames back to back, then ONE skippable frame that holds a seek table. Every zstd decoder
 * decompresses such a stream unchanged (it passes over the skippable frame); a reader that knows the table touches only the frames that cover
 * the range it wants. All fields little-endian:
 *
 *   Skippable_Magic_Number 4  0x184D2A5E
 *   Frame_Size             4  bytes that follow this field: n * E + 9
 *   Seek_Table_Entries   n*E  E = 8, or 12 with checksums: Compressed_Size (4), Decompressed_Size (4), [Checksum (4)]
 *   Number_Of_Frames       4  n <= 2^27
 *   Seek_Table_Descriptor  1  bit 7 = Checksum_Flag; bits 6..2 reserved (written 0, rejected when set); bits 1..0 unused (ignored)
 *   Seekable_Magic_Number  4  0x8F92EAB1
 *
 * Checksum = the low 32 bits of XXH64 (seed 0) of the frame's uncompressed bytes, the value of a frame's own content-checksum trailer. Frame i
 * starts at the sum of Compressed_Size over the entries in front of it; an entry may describe a skippable or an empty frame (Decompressed_Size 0);
 * Decompressed_Size <= 2^30. DESIGN.md section 9 has the decisions. */
#define ZHIP_SEEKABLE_CHECKSUM 1
uint64_t zhip_seekable_frame_count(uint64_t srcSize, uint32_t frameSize);              /* ceil(srcSize / frameSize); 0 for srcSize 0 */
uint64_t zhip_seekable_bound(uint64_t srcSize, uint32_t frameSize, int flags);          /* worst-case stream bytes; 0 = invalid arguments */
/* Cuts [d_src, d_src + srcSize) into chunks of frameSize bytes (a shorter last one), compresses them as ONE batch through zhip_compress_batch_device with the
 * context's level, parameters, flags and dictionary (into zhip_compress_bound-sized slots of context scratch), lays the frames back to back into d_dst and
 * writes the table behind them. frameSize: 1 ... 2^30, at most 2^27 frames, else ZHIP_ERR_UNSUPPORTED. With ZHIP_SEEKABLE_CHECKSUM the entries carry checksums
 * (of the source chunks), whether or not the context's checksumFlag puts trailers into the frames. Asynchronous and stream-ordered under exactly the rules
 * above for zhip_compress_batch_device: no host wait between its kernels except while scratch grows. The context's size hint is left as the caller set it.
 * d_status[0] = 0 or the zstd error code of the lowest failing frame, d_status[1] = that frame's index -- zhip_ctx_sync(ctx, stream, d_status, 1, &err) works on
 * it as it is. A failure sets *d_streamSize = 0 and writes nothing into d_dst: a chunk the context's level refuses (40), a stream that does not fit dstCapacity
 * (70; the index is the first frame that ends beyond it, the last frame where only the table does not fit). Nothing at or beyond d_dst + dstCapacity is ever
 * written. srcSize 0 gives the 17-byte stream of zero frames. */
int zhip_seekable_compress_device(zhip_ctx*, const void* d_src, uint64_t srcSize, uint32_t frameSize, int flags,
                                  void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status /* [2] */, void* stream);

/* One frame per RECORD: d_records[i] = (offset, length) of record i in d_src, a table in DEVICE memory that a kernel queued on `stream` just before the call may
 * have written. The stream holds nRecords frames in index order -- its content is the records concatenated in that order -- and the table behind them; records
 * may lie anywhere in d_src, in any order, with gaps, two may name the same bytes, length 0 is allowed (zhip_compress_batch_device's rule for its segments).
 * Everything else is zhip_seekable_compress_device's: the context's level, parameters, flags and dictionary, ZHIP_SEEKABLE_CHECKSUM (of the source records),
 * one stream-ordered sequence with no host wait except while scratch grows, the context's size hint left as the caller set it.
 * What the host says without waiting: nRecords <= 2^27; maxContentBytes, an upper bound on the sum of the lengths (with nRecords it sizes the slots the records
 * are compressed into: maxContentBytes + (maxContentBytes >> 8) + 80 * nRecords bytes of context scratch, never more than for nRecords records of
 * maxRecordBytes); maxRecordBytes <= 2^30, an upper bound on every length -- the batch's size hint for this call, so a value above 128 KiB selects the
 * several-block paths. Else ZHIP_ERR_UNSUPPORTED. The device checks what the host assumed BEFORE anything is compressed: a length above maxRecordBytes, an
 * offset + length beyond srcSize or one that wraps: 72 (srcSize_wrong) at the lowest such record; none of these, but the lengths sum to more than maxContentBytes:
 * 72 at the lowest record whose running end exceeds it. Behind the batch: the lowest failing frame keeps the compressor's code (40 for a record the level
 * refuses), then the capacity (70; the first frame that ends beyond dstCapacity, the last frame where only the table does not fit). d_status = {code, record
 * index}; every failure sets *d_streamSize = 0 and writes nothing into d_dst; nothing at or beyond d_dst + dstCapacity is ever written. nRecords 0 gives the
 * 17-byte stream of zero frames. */
uint64_t zhip_seekable_records_bound(uint64_t maxContentBytes, uint64_t nRecords, int flags);   /* worst-case stream bytes for nRecords records whose lengths sum to at most maxContentBytes; 0 = invalid arguments */
int zhip_seekable_compress_records_device(zhip_ctx*, const void* d_src, uint64_t srcSize,
                                          const zhip_segment* d_records /* DEVICE: (offset, length) of record i in d_src */, size_t nRecords,
                                          uint64_t maxContentBytes, uint64_t maxRecordBytes, int flags,
                                          void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status /* [2] */, void* stream);

typedef struct zhip_seekable zhip_seekable;
typedef struct { uint64_t streamSize, contentSize; uint32_t nFrames, maxFrameContent; int checksumFlag; } zhip_seekable_info;
/* Reads the table of a stream in HBM (any writer's) and returns a handle for range reads; d_stream is borrowed and must stay as it is while the handle lives.
 * This call MAY WAIT on the host: it reads the 9-byte footer, then the 8-byte skippable header, then a kernel checks every entry and builds the exclusive prefix
 * sums of both size columns in device memory the handle owns. Checked: both magics (a wrong one: ZHIP_ERR_ZSTD with prefix_unknown, 10), and -- each
 * ZHIP_ERR_ZSTD with corruption_detected, 20 -- Frame_Size == n * E + 9, the reserved bits, n <= 2^27, every Decompressed_Size <= 2^30, the sum of
 * Compressed_Size == the table frame's offset (streamSize - 8 - Frame_Size). No handle is created for a stream that fails. After a successful open no
 * offset derived from the table points outside [d_stream, d_stream + streamSize). The handle keeps on the host what the range call needs. */
int  zhip_seekable_open_device(zhip_ctx*, const void* d_stream, uint64_t streamSize, void* stream,
                               zhip_seekable** out, zhip_seekable_info* info, zhip_error* err);
void zhip_seekable_close(zhip_seekable*);      /* waits for the device (it frees device memory) */
/* Content bytes [offset, offset + length) into d_dst. Asynchronous and stream-ordered, no host wait (but where the handle's scratch grows). offset + length
 * beyond contentSize: ZHIP_ERR_SIZE_MISMATCH, both numbers in zhip_last_error(), nothing written. length 0 launches nothing and sets the status to 0. Else the
 * frames that cover the range are decoded as ONE batch through zhip_decompress_batch_device: frames wholly inside the range straight into their place in d_dst,
 * a first and a last frame that the range cuts into the handle's scratch, from where a device copy moves the covered part; entries with Decompressed_Size 0
 * are never handed to the decoder; maxFrameContent above 128 KiB selects the several-block mode for these launches only. A frame that comes out at another
 * size than its entry's fails with 20, with Checksum_Flag a frame whose XXH64 low word differs from its entry's with 22 (checksum_wrong); a frame the decoder
 * refuses keeps the decoder's code. d_status = {code, frame index} of the lowest failing frame, {0, 0} without one. Bytes of d_dst outside [0, length) are untouched.
 * Range calls on one handle follow the context's rule: one host thread and one stream at a time. */
int  zhip_seekable_decompress_device(zhip_ctx*, zhip_seekable*, uint64_t offset, uint64_t length,
                                     void* d_dst /* length bytes */, int32_t* d_status /* [2] */, void* stream);

/* Many ranges in ONE decode batch. ranges is a HOST array, read before the call returns: content bytes [offset, offset + length) go to d_dst + dstOffset.
 * Asynchronous and stream-ordered under the rules of zhip_seekable_decompress_device: one host thread and one stream at a time per handle, no host wait (but
 * where the handle's scratch grows). Checked on the host before anything is queued, and nothing -- d_status included -- is written where a check fails: a range
 * that ends beyond contentSize or wraps, and a dstOffset + length beyond dstCapacity (ZHIP_ERR_SIZE_MISMATCH; zhip_last_error() holds the range's index and both
 * numbers); two ranges of non-zero length whose destinations overlap, NULL arguments and nRanges > 2^27 (ZHIP_ERR_UNSUPPORTED). The overlap check sorts the
 * ranges by dstOffset. Content ranges may overlap, repeat, share frames, come in any order and have length 0 (status {0, 0}, nothing written).
 * Every frame with content that at least one range touches is handed to zhip_decompress_batch_device exactly ONCE per call (stats->items); entries of
 * Decompressed_Size 0 never are. A frame wholly inside exactly one range and touched by no other decodes straight into its place (inPlace); every other frame
 * decodes into the handle's scratch, slots in ascending frame order (scratchBytes: their sizes' sum), and device copies of contiguous spans (copyJobs) move
 * the covered parts to every range that needs them. Where scratchBytes exceeds the handle's scratch limit the item list is cut at frame boundaries into
 * `passes`, each a decode batch of its own queued back to back with no host wait; the scratch never grows beyond max(limit, largest scratch frame).
 * d_status[0 .. 1] = {code, range index} of the lowest-index range that failed ({0, 0}: none; zhip_ctx_sync(ctx, stream, d_status, 1, &err) works on it);
 * d_status[2 + 2r .. 3 + 2r] = {code, frame index} of the lowest failing frame among those range r needs -- what the single-range call reports for it. A failing
 * frame fails only the ranges that need it. No byte of d_dst outside the union of the ranges' destinations is ever written. nRanges 0 sets d_status[0 .. 1]
 * and launches nothing else. The plan's tables travel through pinned memory the handle owns, so the caller's array is free when the call returns. A
 * device-resident range array is not offered: the host must know the batch's item count without a wait. */
typedef struct { uint64_t offset, length, dstOffset; } zhip_seekable_range;
typedef struct { uint64_t items, inPlace, scratchBytes, copyJobs, passes; } zhip_seekable_gather_stats;
int  zhip_seekable_decompress_ranges_device(zhip_ctx*, zhip_seekable*, const zhip_seekable_range* ranges, size_t nRanges,
                                            void* d_dst, uint64_t dstCapacity, int32_t* d_status /* [2 + 2 * nRanges] */,
                                            zhip_seekable_gather_stats* stats /* host, may be NULL; filled before the call returns */, void* stream);
void zhip_seekable_set_scratch_limit(zhip_seekable*, uint64_t bytes);      /* of the many-ranges call; 0 = the default, 1 GiB */
/* The table the handle opened: out[0 .. count] = the decompressed offsets of frames first .. first + count (count + 1 values; frame f is content bytes
 * [out[f - first], out[f - first + 1])), from the handle's host copy: no device work, no wait. first + count beyond nFrames: ZHIP_ERR_SIZE_MISMATCH. */
int  zhip_seekable_frame_offsets(const zhip_seekable*, uint32_t first, uint32_t count, uint64_t* out);
/* Whole frames by index -- records of a stream written by zhip_seekable_compress_records_device, frames of any writer's: frame frames[k]'s content goes to
 * d_dst + dstOffsets[k] or, with dstOffsets NULL, back to back in call order. frames and dstOffsets are HOST arrays, read before the call returns. Every index
 * becomes the range of its frame's content and the call is zhip_seekable_decompress_ranges_device's from there: its checks (destinations beyond dstCapacity,
 * overlapping destinations), its stream order, its d_status layout with positions for ranges, its guards, its stats. Every distinct frame is decoded once; a
 * frame named once decodes straight into its place (inPlace == items where the indices are distinct), a frame named more than once goes through the handle's
 * scratch; an empty frame yields {0, 0} and no item. An index >= nFrames: ZHIP_ERR_SIZE_MISMATCH with the position in zhip_last_error(), nothing queued. */
int  zhip_seekable_decompress_frames_device(zhip_ctx*, zhip_seekable*, const uint32_t* frames, size_t nFrames,
                                            const uint64_t* dstOffsets /* host, may be NULL */, void* d_dst, uint64_t dstCapacity,
                                            int32_t* d_status /* [2 + 2 * nFrames] */, zhip_seekable_gather_stats* stats, void* stream);

/* EDIT: a new stream out of frames of an opened one and of new records -- append, replace, drop, reorder, repeat -- without recompressing what is kept. The new
 * stream holds nPicks frames in pick order and the table behind them. A ZHIP_PICK_FRAME pick is frame `index` of `old`: its bytes verbatim and its table entry
 * as it is, checksum word included -- any writer's frame, empty, skippable, of several blocks, of another level or dictionary; nothing looks inside it. A
 * ZHIP_PICK_RECORD pick is record `index` of d_records, compressed exactly as zhip_seekable_compress_records_device compresses it: the context's level,
 * parameters, flags, dictionary and match finder, maxRecordBytes the size hint for this call only, the same pre-check (72). A frame or a record may be picked
 * any number of times; a record nobody picks is compressed and dropped; zero picks give the 17-byte stream. With old == NULL and picks RECORD 0 .. n-1 the
 * stream is the records call's byte for byte. picks is a HOST array, read before the call returns: it travels through pinned memory the handle owns (the
 * context, without a handle). A device-resident pick list is not offered: the host must know the item counts without a wait.
 * Checksums: with `old` the new table carries checksum words exactly when the old one does, and flags & ZHIP_SEEKABLE_CHECKSUM must say the same (else
 * ZHIP_ERR_UNSUPPORTED); a new record's word is the XXH64 low word of its source bytes; with old == NULL the flag decides.
 * Checked on the host before anything is queued, and nothing -- d_status included -- is written where a check fails: NULL arguments, nPicks > 2^27, a pick that
 * is neither kind, a FRAME pick with old == NULL, the records call's bounds on nRecords and maxRecordBytes (ZHIP_ERR_UNSUPPORTED); a frame index >= nFrames or
 * a record index >= nRecords (ZHIP_ERR_SIZE_MISMATCH, the position in zhip_last_error()); [d_dst, d_dst + dstCapacity) overlapping the old stream
 * (ZHIP_ERR_UNSUPPORTED) -- but for the one form that is APPEND IN PLACE: d_dst is the old stream's base and the picks begin with FRAME 0 .. nFrames-1 in order.
 * Then the kept frames are neither read nor written, the new frames start where the old table started (its entries are kept aside in context scratch first),
 * and the buffer must have room for the bound. After a successful append in place the handle describes bytes that no longer exist: close it and open the
 * stream again before any other call on it.
 * Asynchronous and stream-ordered under the rules of the other seekable calls, no host wait except while scratch grows. d_status = {code, index}, and
 * zhip_ctx_sync(ctx, stream, d_status, 1, &err) works on it: 72 from the records' pre-check with the RECORD index; else the lowest pick POSITION whose record the
 * compressor refused keeps its code (40); else the capacity: 70 at the first pick whose frame ends beyond dstCapacity, the last pick where only the table does
 * not fit. Every failure sets *d_streamSize = 0 and writes nothing into d_dst -- in place the old stream, table included, is intact and readable. Nothing at
 * or beyond d_dst + dstCapacity is ever written.
 * zhip_seekable_edit_bound: the kept picks' compressed sizes (from the handle's host copy of the table: no wait) + zhip_compress_bound(maxRecordBytes) per
 * RECORD pick + the table; 0 for arguments the edit call would refuse on sight (record indices are not checked: the bound does not know nRecords). */
enum { ZHIP_PICK_FRAME = 0, ZHIP_PICK_RECORD = 1 };
typedef struct { uint32_t from, index; } zhip_seekable_pick;   /* frame `index` of the opened stream, kept as it is; or record `index` of d_records, compressed by this call */
uint64_t zhip_seekable_edit_bound(const zhip_seekable* old, const zhip_seekable_pick* picks, size_t nPicks, uint64_t maxRecordBytes, int flags);
int zhip_seekable_edit_device(zhip_ctx*, zhip_seekable* old /* may be NULL */,
                              const zhip_seekable_pick* picks /* HOST, read before the call returns */, size_t nPicks,
                              const void* d_src, uint64_t srcSize, const zhip_segment* d_records /* DEVICE */, size_t nRecords,
                              uint64_t maxContentBytes, uint64_t maxRecordBytes, int flags,
                              void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status /* [2] */, void* stream);

/* TYPED STREAMS: a tensor of elementSize-byte elements (2, 4 or 8) stored as one BYTE PLANE per frame, so that every byte position of the elements gets
 * entropy tables of its own. frameSize keeps its meaning as the content bytes of one frame; it is the number of elements of one GROUP. The source
 * (srcSize a multiple of elementSize) is cut into groups of frameSize elements, a last one of e <= frameSize; group g becomes the elementSize frames
 * g * elementSize + p, frame g * elementSize + p holding byte p of every element of the group in element order. Behind the last plane frame stands the MARKER,
 * a skippable frame of 24 bytes -- magic 0x184D2A5D, Frame_Size 16, then four little-endian words: 'Z' 'H' 'P' 'L', version 1, elementSize, frameSize -- with a
 * seek-table entry of its own (Compressed_Size 24, Decompressed_Size 0, with checksums 0x51D8E999: the low word of XXH64 of nothing); the standard table is last.
 * The stream stays an ordinary seekable stream: the table's sizes sum to the content size, the checksums are those of the plane frames' content, and every
 * zstd decoder -- zhip_seekable_decompress_device, _ranges_, _frames_ and zhip_seekable_edit_device on a typed handle included -- sees its literal, PLANAR
 * content. Only zhip_seekable_decompress_typed_ranges_device puts the elements back together.
 *
 * zhip_planes_split_device / zhip_planes_join_device are the two transposition kernels on their own, over whole buffers of `size` bytes: split writes group
 * g's plane p to d_dst + g * elementSize * frameSize + p * e_g, join is its inverse. Asynchronous, stream-ordered, no wait, no memory taken. d_src and d_dst
 * must not overlap. ZHIP_ERR_UNSUPPORTED: an elementSize other than 2, 4, 8, a size that is no multiple of it, frameSize 0 or above 2^30.
 *
 * zhip_seekable_compress_typed_device: the split kernel writes a planar copy of the source into context scratch (srcSize bytes, kept between calls like the
 * other areas) with the record table of the n * elementSize planes, zhip_seekable_compress_records_device's sequence compresses them as they are (so the
 * frames are byte for byte libzstd's frames of the planes; under the wave match finder valid but not libzstd's, as for every call), and two small kernels put
 * the marker in. The status, the failure rules and the guards are the records call's; a stream whose marker and entry do not fit dstCapacity fails with 70 like
 * one whose table does not. elementSize 1 is zhip_seekable_compress_device, the same bytes. ZHIP_ERR_UNSUPPORTED beyond the plain call's: elementSize not in
 * {1, 2, 4, 8}, srcSize no multiple of it, frameSize 0 or above 2^30, more than 2^27 - 1 plane frames.
 * zhip_seekable_typed_bound: the records bound for the plane frames, plus the marker and its entry; 0 = invalid arguments.
 *
 * zhip_seekable_open_device recognises a typed stream: where the last entry is (24, 0) it reads those 24 bytes (the one extra copy and wait, only then). No
 * tag: a plain stream. A tag with version 1, an elementSize of 2, 4 or 8 and frames that are whole groups of equally sized planes, frameSize elements each but
 * for a shorter last group: a typed one. A tag and anything else: ZHIP_ERR_ZSTD with corruption_detected (20) at the first frame that does not fit.
 * zhip_seekable_element_size: 1 for a plain stream; zhip_seekable_group_elements: frameSize (0 for a plain stream).
 *
 * zhip_seekable_decompress_typed_ranges_device: zhip_seekable_decompress_ranges_device in ELEMENT order -- offsets and lengths count bytes of the tensor, may
 * start and end inside an element, overlap, repeat, come in any order, be empty; the same host checks, the same d_status shape ({code, range index}, then per
 * range {code, frame index} of the first failing plane frame among those it needs), the same guards. The host plans planar ranges (a run of whole groups is
 * one, a partly covered group elementSize of them, rounded out to whole elements), the many-ranges call decodes them into a planar buffer the handle owns, the
 * join kernel moves the elements to d_dst. The planar buffer is bounded by the handle's scratch limit: ranges are taken in passes and cut at group boundaries;
 * one piece above the limit is held whole. stats: the sums over the passes' many-ranges calls, `passes` the typed passes. A plain handle: ZHIP_ERR_UNSUPPORTED. */
int      zhip_planes_split_device(zhip_ctx*, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, void* d_dst, void* stream);
int      zhip_planes_join_device(zhip_ctx*, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, void* d_dst, void* stream);
uint64_t zhip_seekable_typed_bound(uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, int flags);
int      zhip_seekable_compress_typed_device(zhip_ctx*, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, int flags,
                                             void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status /* [2] */, void* stream);
uint32_t zhip_seekable_element_size(const zhip_seekable*);
uint32_t zhip_seekable_group_elements(const zhip_seekable*);
int      zhip_seekable_decompress_typed_ranges_device(zhip_ctx*, zhip_seekable*, const zhip_seekable_range* ranges, size_t nRanges,
                                                      void* d_dst, uint64_t dstCapacity, int32_t* d_status /* [2 + 2 * nRanges] */,
                                                      zhip_seekable_gather_stats* stats /* host, may be NULL */, void* stream);

/* FILTERS of a typed stream: what is done to a group's elements before the plane split. ZHIP_FILTER_DELTA is for integer tensors whose
 * neighbours are close -- offsets, sorted ids, timestamps, counters, running sums: each element's bit pattern is read as an unsigned little-endian integer of
 * 8 * elementSize bits, and per group d[0] = x[0], d[i] = x[i] - x[i - 1] mod 2^(8 * elementSize); the plane frames hold the byte planes of d. Groups stay
 * independent, so a group is still the unit of random access. Floats gain nothing from it. Everything else about a typed stream is unchanged: the frames are
 * libzstd's frames of those planes, the table's checksums are those of the planar content, zstd -d and every plain reader see the filtered planar bytes.
 * The marker keeps version 1; its word at +16 is elementSize | filter << 8, so an unfiltered stream is byte for byte what it was, and a reader from before
 * the filters refuses a filtered stream as an element size it does not know. Any value but 0, 1 or 4 (ZHIP_FILTER_XOR_BASE, below) in bits 8 .. 31 is a marker this reader does not
 * understand: corruption_detected (20) at the marker frame.
 *
 * zhip_planes_split_filter_device / zhip_planes_join_filter_device: the transposition kernels with the filter fused in. Split subtracts on the words between
 * its loads and its stores (no pass of its own over the source); join under ZHIP_FILTER_DELTA is the inclusive prefix sum of every group and runs as three
 * launches -- tile sums, their exclusive prefix sums per group, join-scan-store -- with a uint64 per 1 024 elements of context memory, kept between calls.
 * zhip_seekable_compress_typed_filter_device: zhip_seekable_compress_typed_device with the filter in the split and in the marker.
 * With ZHIP_FILTER_NONE all three are the calls without a filter, byte for byte and launch for launch. ZHIP_ERR_UNSUPPORTED, with nothing queued and nothing
 * written, beyond those calls': a filter that is neither, and a filter other than ZHIP_FILTER_NONE with elementSize 1. zhip_seekable_typed_bound holds for
 * every filter (a filter changes no size bound).
 * zhip_seekable_filter: the opened stream's filter (0 for a plain stream). zhip_seekable_decompress_typed_ranges_device returns the ELEMENTS of a filtered
 * stream with no new argument: a group a range covers in part is fetched from its first element (its planes' ranges start at the planes' starts), the join
 * sums over what is in front and stores the range only. The plane frames are decoded whole either way, so the decode costs what it did; the copy out of the
 * decode scratch and the join grow by the elements in front of the range within its group. */
enum { ZHIP_FILTER_NONE = 0, ZHIP_FILTER_DELTA = 1 };
int      zhip_planes_split_filter_device(zhip_ctx*, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, uint32_t filter, void* d_dst, void* stream);
int      zhip_planes_join_filter_device(zhip_ctx*, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, uint32_t filter, void* d_dst, void* stream);
int      zhip_seekable_compress_typed_filter_device(zhip_ctx*, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, uint32_t filter, int flags,
                                                    void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status /* [2] */, void* stream);
uint32_t zhip_seekable_filter(const zhip_seekable*);

/* ZHIP_FILTER_XOR_BASE: the filter for VERSIONS of one tensor -- checkpoint after checkpoint, a fine-tune beside its base model, an optimizer
 * state some steps later. The caller holds a BASE of the source's size in device memory (the previous checkpoint), and the plane frames hold the byte planes
 * of x[i] ^ b[i]: the elements' bit patterns XORed bytewise, so nothing depends on the byte order within an element, there are no carries, and a byte needs
 * its base byte and nothing else -- a range that starts inside a group is fetched from where it starts (no elements in front, unlike delta). Versions differ
 * in the low mantissa bits and almost nowhere else: the high planes become runs of zeros, the low planes stay noise (what ZHIP_FINDER_AUTO sorts per frame).
 * The frames are libzstd's frames of those planes, the table's checksums those of the filtered planar content, zstd -d and every plain reader
 * (zhip_seekable_decompress_device, _ranges_, _frames_, zhip_seekable_edit_device) see the filtered planar bytes. The marker keeps version 1, its word at
 * +16 is elementSize | 4 << 8. Filter values 2 and 3 are none and stay refused everywhere.
 *
 * THE STREAM DOES NOT NAME ITS BASE. Reading it with another tensor of the right size returns wrong elements with status 0; keeping stream and base together
 * is the caller's business (a fingerprint of the base is not part of the format). The calls here XOR once; a chain of versions is read by
 * zhip_seekable_decompress_typed_ranges_chain_device below.
 *
 * zhip_planes_split_base_device / zhip_planes_join_base_device: the transposition kernels with the XOR fused in, one kernel each way; d_base is `size` bytes.
 * zhip_seekable_compress_typed_base_device: zhip_seekable_compress_typed_device with the XOR in the split and filter 4 in the marker; d_base is srcSize bytes.
 * zhip_seekable_decompress_typed_ranges_base_device: zhip_seekable_decompress_typed_ranges_device for a filter-4 handle -- the same plan, passes and scratch
 * limit, the base XORed in by the join; d_base is baseSize bytes, the stream's content size, of which only the bytes at the content offsets the ranges cover
 * are read. ZHIP_ERR_UNSUPPORTED, with nothing queued and nothing written, beyond the calls' own refusals: a NULL base; elementSize 1; a baseSize other than
 * the stream's content size; a base that shares a byte with the output (d_dst over size / dstCapacity / dstCapacity bytes); the read with a base on a handle
 * whose filter is not 4; and zhip_seekable_decompress_typed_ranges_device (no base) on a filter-4 handle. The three *_filter_device calls refuse filter 4 as
 * they refuse 2: they have no base to take. */
enum { ZHIP_FILTER_XOR_BASE = 4 };
int      zhip_planes_split_base_device(zhip_ctx*, const void* d_src, uint64_t size, uint32_t elementSize, uint32_t frameSize, const void* d_base, void* d_dst, void* stream);
int      zhip_planes_join_base_device(zhip_ctx*, const void* d_planar, uint64_t size, uint32_t elementSize, uint32_t frameSize, const void* d_base, void* d_dst, void* stream);
int      zhip_seekable_compress_typed_base_device(zhip_ctx*, const void* d_src, uint64_t srcSize, uint32_t frameSize, uint32_t elementSize, const void* d_base, int flags,
                                                  void* d_dst, uint64_t dstCapacity, uint64_t* d_streamSize, int32_t* d_status /* [2] */, void* stream);
int      zhip_seekable_decompress_typed_ranges_base_device(zhip_ctx*, zhip_seekable*, const void* d_base, uint64_t baseSize, const zhip_seekable_range* ranges, size_t nRanges,
                                                           void* d_out, uint64_t outCapacity, int32_t* d_status /* [2 + 2 * nRanges] */,
                                                           zhip_seekable_gather_stats* stats /* host, may be NULL */, void* stream);

/* CHAINS of xor-with-base streams. A store of versions v0, v1, ... of one tensor writes every version against its PREDECESSOR (the smaller the
 * step, the smaller the stream): v0 as a full unfiltered typed stream, v(i) as zhip_seekable_compress_typed_base_device(v(i), base = v(i-1)). Elements of
 * version n are then v0 ^ d1 ^ ... ^ dn. zhip_seekable_decompress_typed_ranges_chain_device reads ranges of them in one call from links = [full, d1, ..., dn]
 * with d_base NULL, or from links = [d1, ..., dn] and d_base = v0 (baseSize its bytes, the content size): ONE plan from link 0's table and scratch limit, per
 * pass one many-ranges call per link -- only the frames the ranges touch are decoded, into that link's own planar scratch -- and ONE join kernel that XORs all
 * links' planar words, transposes once, XORs the base and writes the output. Nothing intermediate is written. Traffic per element byte: nLinks planar reads,
 * a base read where there is one, one write (following the chain by hand: 3 per link). Scratch: every link holds at most link 0's scratch limit of planar
 * bytes (or one piece above it), the chain at most nLinks times that. nLinks == 1 returns byte for byte what the single-stream calls return.
 * d_status [2 + 2 * nRanges] has the layout and meaning of zhip_seekable_decompress_typed_ranges_device's. A range fails if any link's frames under it
 * failed; where several links fail, the EARLIEST link in chain order is reported, the frame index being the index in THAT link's frame table.
 * d_link [1 + nRanges] (may be NULL): [0] the link behind d_status[0 .. 1], [1 + r] the link whose frame failed range r, -1 where none did. A failed range's
 * bytes are unspecified, every other range is exact. stats sums over all links' many-ranges calls, `passes` counting the typed passes once.
 * ZHIP_ERR_UNSUPPORTED, nothing queued, nothing written, the message naming the link: nLinks 0 or above 16; a NULL link; a handle that appears twice (its
 * planar scratch would be shared); a plain link (element size 1); links that differ in element size, group elements or content size; link 0 with the delta
 * filter; a later link whose filter is not 4; link 0 with filter 4 and no base; link 0 unfiltered WITH a base; a baseSize other than the content size; a base
 * that shares a byte with the output; and the ranges' own refusals. The handles are used by the call: as with every call on a handle, one call at a time.
 * NO LINK NAMES ITS BASE OR ITS PREDECESSOR: a chain in the wrong order, or with a link of another tensor of the same shape, returns wrong elements with
 * status 0. (XOR commutes, so the order of the links behind a correct start does not matter; leaving one out or taking a foreign one does.)
 * zhip_planes_join_chain_device: the join kernel on its own over nLinks whole planar buffers of `size` bytes (zhip_planes_split_*'s layout), d_base NULL or
 * `size` bytes that share none with d_dst. */
enum { ZHIP_CHAIN_MAX = 16 };
int      zhip_planes_join_chain_device(zhip_ctx*, const void* const* d_planar /* host array [nLinks] of device pointers */, size_t nLinks, uint64_t size, uint32_t elementSize,
                                       uint32_t frameSize, const void* d_base /* may be NULL */, void* d_dst, void* stream);
int      zhip_seekable_decompress_typed_ranges_chain_device(zhip_ctx*, zhip_seekable* const* links /* host array, oldest first */, size_t nLinks,
                                                            const void* d_base /* NULL iff link 0 is unfiltered */, uint64_t baseSize,
                                                            const zhip_seekable_range* ranges, size_t nRanges, void* d_out, uint64_t outCapacity,
                                                            int32_t* d_status /* [2 + 2 * nRanges] */, int32_t* d_link /* [1 + nRanges], may be NULL */,
                                                            zhip_seekable_gather_stats* stats /* host, may be NULL */, void* stream);

/* name of a kernel as it appears in rocprofv3 traces ("" past the last one), and its average duration (ms) over the launches since the last call, measured with HIP events
 * on the stream it is launched on (for bench.py's roofline). k: 0 / 1 the generic decode / encode kernels, 2 K1 (with K0 and the bin pass in front of / behind it), 3 K2,
 * 4 K3, 5 / 6 the lane-serial match kernel (the greedy strategy's zhip_encode_match_greedy_kernel where that runs in its place) and the entropy kernel, 7 K1b -- which runs BESIDE K2 on a side stream: timed from K2's end to its own end, what it adds to the step --,
 * 8 the flat match kernel -- the match stage of a chunk whichever of its forms ran: the double-fast search's and, since the fast strategy has a flat search of its own
 * (levels 1, 2 and negative levels without a dictionary, sources of one block), that one's; the LDS-source kernels of small batches too --, 9 "zhip_decode_pipeline_span": not a kernel, a chunk's decode pipeline from K1's start to K3's end (what the overlapping kernels cost together),
 * 10 the wave match kernel (ZHIP_FINDER_WAVE: once per chunk, with 5 and 8 at zero launches),
 * 11 the literals-only kernel (ZHIP_FINDER_NONE: once per chunk, timed with the trailer kernel behind it, with 5, 6, 8 and 10 at zero launches),
 * 12 the classify kernel (ZHIP_FINDER_AUTO and zhip_classify_batch_device: once per chunk of 65 536 sources; under ZHIP_FINDER_AUTO the two parts' kernels count in their own
 * directions, so a batch that is all one kind shows zero launches of the other kind). */
const char* zhip_kernel_name(int k);
int         zhip_ctx_kernel_time(zhip_ctx*, int direction, double* avgMs, uint64_t* launches);
/* how many frames of the context's last zhip_decompress_batch_device call the phase-split kernels (K1 -> K2 -> K3) handed to the generic kernel: frames of several
 * blocks outside the several-block mode, frames that found the chunk's item slots or arenas used up, offsets the packed sequences cannot hold. Waits for the device
 * (for tests and tuning: a batch that should take the pipeline and does not is correct and slow). */
int         zhip_ctx_decode_fallbacks(zhip_ctx*, uint64_t* frames);
/* the compress direction's table placement pick (zhip_compress_batch_device: the first launch of 16 384 frames or more -- 49 152 until round 6's last session -- times the match kernel on
 * up to three table allocations held side by side and keeps the fastest; where a probe is cheap -- dictionary batches -- and the three came out alike, up to three more):
 * ms3[k] = candidate k's PROBE time in ms for the first three (0 = not tried) -- since round 6's last session a probe launch searches the first 8 KiB of every source only, which ranks the
 * allocations like the whole launch does at a thirteenth of the time (30 against 36 ms per 65 536 sources of 128 KiB where the whole launches take 407 against 470). Returns the index kept (0..7: eight candidates are probed since round 6's last session -- one allocation in eight was a third, faster kind, 388-392 ms where the usual fast kind takes 406-417). */
int         zhip_ctx_table_pick(zhip_ctx*, float* ms3);

#ifdef __cplusplus
}
#endif
#endif
