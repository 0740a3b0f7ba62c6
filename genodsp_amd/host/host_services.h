/* host_services.h -- driver internals shared with the operator files (not part of the
 * plugin surface in include/genodsp_interface.h). */
#ifndef host_services_H
#define host_services_H

#include "genodsp_interface.h"
#include "genodsp_hip.h"

extern int selectStrategy;                  /* GDSP_SELECT_* (--percentile=) */
extern int firMode;                         /* GDSP_FIR_EXACT or GDSP_FIR_FMA (--smooth=) */
extern int dbgInput;                        /* --debug=input: echo every input line (genodsp.c:1422) */

/* pending-interval batches: collect in file order, apply on the owning device */
void ib_begin       (void);
void ib_add         (spec* s, u32 start, u32 end, valtype val);
u64  ib_pending     (void);
void ib_flush_apply (int overlapOp, int clearFlags, valtype missingVal, int everyChromosome);
void ib_flush_apply_partner (int overlapOp, int clearFlags, valtype missingVal, int everyChromosome);   /* into partner_of() */
void ib_flush_scale (int divide, valtype infinityVal);
void ib_flush_mask  (int inside, valtype outsideVal, int binarizeFirst);
void ib_flush_over  (int wantMax, valtype fillVal);

void sync_all_devices    (void);
/* the signal as the stretches someone answers for, wherever it lives now: whole chromosomes, or (--sharding=bases,
 * between ingest and report) stretches of them.  v[0] is base `first` of chromosome s->chrom; base/baseLen is the
 * 16-byte aligned vector v lies in (an elementwise operator may as well run over all of it) */
typedef struct sigpart { spec* s;  valtype* v;  u32 n;  u32 first;  valtype* base;  u32 baseLen; } sigpart;
int  signal_parts (sigpart** parts);
int  signal_in_whole_chromosomes (void);       /* false under --sharding=bases (the signal may live in stretches) */
void to_whole (void);                          /* make the whole chromosomes current (file-driven operators, report) */
/* how whole-genome operators (percentile, invert) combine what the devices of this process found: the
 * reduction hook for gdsp_percentiles (NULL: the library adds its devices' counts on the host) */
gdsp_reduce_fn reduce_over_devices (void** ctx);
void genome_extremes (valtype* lo, valtype* hi);     /* min / max of the whole genome over all devices (invert) */
u64   ib_batch_limit (void);                   /* intervals buffered before they are applied (8 M; GDSP_BATCH_INTERVALS) */
void* device_workspace (size_t bytes);         /* per-device, grows on demand, kept for the run */
void* long_window_workspace (size_t* bytes);   /* lazily allocated, for windows beyond one LDS tile */
int  device_count_in_use (void);
int  device_index_of     (spec* s);
int  physical_device_of  (spec* s);
double now_ms (void);                          /* the monotonic clock, in milliseconds */

/* ops_common.c: helpers shared by the operator files */
void* new_op           (char* name, size_t bytes, int atRandom);   /* zeroed control record */
void* must_alloc       (void* p, const char* name);                /* p, or the run ends with "out of memory" when it is NULL */
int   origin_opt_take  (char* arg, int* originOne);                /* --origin=one|1|zero|0 */
int   value_column_take (char* name, char* arg, int* valColumn);   /* --value=<col>, --novalue, --novalues, --value=none */
u32   window_arg       (char* name, char* arg, char* argVal, const char* what);
/* "--x=<value|variable>": number now, or a named variable resolved at first apply */
void  value_or_variable (char* argVal, valtype* val, char** varName);
void  resolve_variable  (dspop* op, char** varName, valtype* val, const char* role);
/* the same for a level: a number that is not NaN, or what can be a variable's name; anything else is refused at once */
void  level_arg         (char* name, char* arg, char* argVal, valtype* val, char** varName);
/* what percentile, stats, normalize, histogram and statsover let the user say about the sample and its report; init
 * gives today's defaults (the named global windowSize, 0 meaning 1; no limits; every digit; not quiet), take consumes
 * --min= / --max= and those of the other options that `accepts` names, with the complaints they have always made */
typedef struct sample_opts { u32 window;  valtype minAllowed, maxAllowed;  int precision, quiet; } sample_opts;
#define SAMPLE_OPT_WINDOW    1
#define SAMPLE_OPT_PRECISION 2
#define SAMPLE_OPT_QUIET     4
void  sample_opts_init  (sample_opts* o);
int   sample_opts_take  (sample_opts* o, char* name, char* arg, int accepts);
int   signal_sources    (char* name, gdsp_xsum_source** sources);   /* signal_parts() as the library's source table */
int   place_interval    (char* name, char* filename, char* chrom, spec* s, u32 start, u32 end, u32* adjStart, u32* adjEnd);
int   format_value      (char* text, size_t size, valtype v, int precision);   /* %.17g when precision < 0 */
FILE* open_table        (char* name, char* filename);               /* --output=<file>, or stdout */
void  close_table       (FILE* out);
/* the numbers of a table (statsover, segments), written at p; -> behind what was written.  put_value: format_value's text,
 * at most 400 characters of it, by hand where that gives printf's characters (integers below 10^15, fixed point) */
char* put_unsigned      (char* p, unsigned long long u);
char* put_value         (char* p, valtype v, int precision);
/* count, sum and then mean, min, max, summit or four NA, each behind a tab, and the newline: at most 1647 characters */
char* put_interval_figures (char* p, const gdsp_interval_stat* stat, u32 chromStart, int originOne, int precision);

/* what profileover and matrixover share: the options that name the anchors of a file and the offsets around them
 * (--flank= | --upstream= --downstream=, --bin=, --anchor=, --strand=, --origin=, and the refusal of a window), the
 * complaints of the finished command line (check sets upstream and downstream), and the reader of the file: every
 * interval gives one anchor, from the interval as the file has it; an anchor outside its chromosome's vector is skipped
 * and counted.  anc[i] are the anchors of parts[i], as the library takes them */
enum { anchor_start = 0, anchor_end = 1, anchor_center = 2 };
typedef struct anchor_opts
	{
	int       originOne;
	int       haveFlank, haveUp, haveDown;
	long long flank, upstream, downstream;
	int       anchor, strandColumn;           /* strandColumn: zero-based, -1 when every anchor is plus */
	long long bin;
	} anchor_opts;
typedef struct anchors { u32 *pos, *minus;  u32 count, cap; } anchors;
typedef void (*anchor_used_fn) (void* ctx, int part, u32 index, u32 start, u32 end, int minus);   /* start, end: as the file has them */
void  anchor_opts_init  (anchor_opts* o);
int   anchor_opts_take  (anchor_opts* o, char* name, char* arg);
void  anchor_opts_check (anchor_opts* o, char* name);
int   read_anchor_line  (char* name, char* filename, FILE* f, char* line, int lineLen, u64* lineNumber, int strandCol,
                         char** chrom, u32* start, u32* end, int* minus);
long long anchor_of     (long long s, long long e, int minus, int anchor);
void  read_anchor_file  (char* name, char* filename, const anchor_opts* o, const sigpart* parts, int nsrc, anchors* anc,
                         u64* numRead, u64* numUsed, u64* numSkipped, anchor_used_fn used, void* usedCtx);
/* what matrixover and regionsover share (ops_common.c): a table with one line per used row of a file (an anchor, a
 * region), in the file's order, held whole on the host.  --as= and the names of the figures (GDSP_MATRIX_*); the used
 * rows as their lines name them (length: regionsover's); the refusal of more than ROW_TABLE_MAX_CELLS cells (complaint:
 * the printf format of name, rows, columns, cells and the most cells); a part's vector, device, stream and the storage of
 * its rows (selects the part's device); the lines -- chrom start end strand, the length when withLength, then ncols values,
 * NA where there is none; and the variables and the report at the end */
#define ROW_TABLE_MAX_CELLS (1ull << 30)
extern const char* const figureNames[5];
typedef struct rowrec { u32 part, index, start, end, length;  int minus; } rowrec;
typedef struct rowlist { rowrec* rows;  u64 count, cap;  char* name; } rowlist;
int   figure_opt_take   (char* name, char* arg, int* what);
void  rowlist_add       (rowlist* l, int part, u32 index, u32 start, u32 end, u32 length, int minus);
u64   row_table_cells   (char* name, u64 numUsed, u32 ncols, const char* complaint);
double* row_table_part  (char* name, const sigpart* part, u32 count, u32 ncols, const valtype** d_v, u32* n, int* device, void** stream);
void  row_table_print   (char* name, FILE* out, const rowlist* list, double* const* table, u32 ncols, const sigpart* parts,
                         int strandColumn, int withLength, int precision);
void  row_table_report  (char* rowsName, u64 numUsed, u64 cells, int quiet);

/* ops_fused.c: run op (and the operators after it, up to stopOp) as one fused kernel when
 * the chain is one the device library fuses; returns how many operators were consumed (0 = none) */
int   try_fused_apply   (dspop* op, dspop* stopOp, spec* s);
/* one launch per operator per device (see ops_fused.c) */
int   op_batchable          (dspop* op);
int   op_reach              (dspop* op, u32* left, u32* right);    /* the operator's reach (optraits), false: none */
int   batch_apply_on_device (dspop* op, dspop* stopOp, spec** units, int nunits, int allowFusion);
valtype* partner_of    (spec* s);              /* the second HBM buffer of a chromosome or stretch */
void     flip_spec     (spec* s);              /* swap vector and partner */
void     apply_to_unit (dspop* op, spec* s);   /* the operator's own apply on one chromosome or stretch */
void  op_limits_describe    (dspop* op, int* haveMin, valtype* lo, int* haveMax, valtype* hi, int* keepInside, valtype* zero);
valtype op_add_constant_value (dspop* op);
u32   op_smooth_window    (dspop* op);
u32   op_best_window      (dspop* op);
void  op_morph_reach      (dspop* op, u32* left, u32* right);
void  op_local_describe   (dspop* op, u32* neighborhood, int* wantMax, valtype* fill);
void  op_morph_describe   (dspop* op, u32* left, u32* right, valtype* T, valtype* one, valtype* zero);
void  op_binarize_describe (dspop* op, valtype* T, int* tiesAbove, valtype* one, valtype* zero);
const char* op_binarize_pending (dspop* op, int* tiesAbove, valtype* one, valtype* zero);
/* `= percentile P = binarize --threshold=percentileP` in one read of the signal: runs the percentile operator and, when the
 * operator after it is that binarize, the binarize with it; returns how many operators ran (1 or 2) */
int   percentile_with_binarize (dspop* percentile, dspop* next);

/* ops_percentile.c: a percentile as given on the command line -> thousandths of a percent (0 .. 100000) */
u32   to_thousandths      (valtype pct);
void  percentile_name     (char* varName, u32 percentile);   /* "percentile99", "percentile99.5": the variable of that P (ops_percentile.c) */
/* what the driver knows about an operator, said once, beside the operator, and found by its apply function (traits_of).
 * An operator nobody described (a plugin's) gets the defaults: it may ask for a partner, needs its chromosome in one piece,
 * has no one-launch form, and as a stop operator takes whole chromosomes and is credited the genome's bases at 16 B each */
typedef struct optraits
	{
	opfunc_apply apply;            /* whose traits these are */
	int   inPlace;                 /* never asks for a partner (a one-launch form then gets d_in NULL, d_out the vector) */
	int   onParts;                 /* stop operator that takes the signal's parts as they are (no to_whole()) */
	/* --sharding=bases: true when output i depends on inputs [i-left, i+right] only and not on where i lies in the vector
	 * (so a stretch of a chromosome with that much halo computes what the whole chromosome would); NULL for running
	 * sums, window grids and clump, which need the chromosome in one piece */
	int   (*reach) (dspop* op, u32* left, u32* right);
	int   (*batch) (dspop* op, const gdsp_batch_item* items, int nitems, void* stream);   /* one launch per device; NULL: none */
	/* --report=gpu, stop operators: bytes per base, and the bases when they are not the genome's; NULL: 16 */
	void  (*work)  (dspop* op, u64* bases, double* bytesPerBase);
	} optraits;
/* an operator group beyond the reference's: its rows of the operator table (aliases included), its operators' traits, and
 * where its library half takes the RCCL communicator (NULL: it reduces nothing).  Each group is defined in its own
 * ops_*.c; the driver holds weak references to them, so a build from a shorter source list simply lacks the group */
typedef struct opgroup
	{
	const dspinfo*  rows;    int nrows;
	const optraits* traits;  int ntraits;
	int (*useComm) (gdsp_comm* comm);
	} opgroup;
#define OPGROUP(rows, traits, useComm) \
	{ rows, (int) (sizeof(rows)/sizeof(rows[0])), traits, (int) (sizeof(traits)/sizeof(traits[0])), useComm }
const optraits* traits_of (dspop* op);        /* NULL: nobody described it */
extern const optraits coreTraits[];           /* ops_fused.c: the reference's operators */
extern const int      coreTraitsLen;
int   reach_none    (dspop* op, u32* left, u32* right);   /* per-base operators: 0, 0 */
int   reach_centred (u32 W, u32* left, u32* right);       /* bestmax's window: (W-1)/2 left, the rest right */
/* what segments and keepsegments (ops_keepsegments.c) share: the options that select the segments and shape their
 * table, parsed in one place, and the pass itself.  take: true when `arg` was one of them; take_other: --debug, the
 * complaint about an unknown option, the threshold as a bare number.  segments_run with `paint`: every chromosome's
 * partner is painted from the kept segments (gdsp_keep_segments_batch) and becomes the signal; the table is written
 * when wantTable (to o->outFilename, else stdout); the variables segments, covered and longest are set either way */
typedef struct segments_opts
	{
	char*   thresholdVarName;  valtype threshold;  int haveThreshold, tiesAbove;           /* (as binarize) */
	u32     mergeGap, minLength;
	int     haveMinHeight;  char* minHeightVarName;  valtype minHeight;
	char*   outFilename;
	int     precision, originOne;
	} segments_opts;
typedef struct segments_paint { int mode;  valtype one, zero; } segments_paint;       /* mode: GDSP_KEEP_* */
void  segments_opts_init       (segments_opts* o);
int   segments_threshold_take  (segments_opts* o, char* name, char* arg);   /* --threshold= / T=, --ties: alone (distance) */
int   segments_opts_take       (segments_opts* o, char* name, char* arg);
void  segments_opts_take_other (segments_opts* o, char* name, char* arg);
void  segments_opts_free       (segments_opts* o);
void  segments_run             (dspop* op, segments_opts* o, int wantTable, const segments_paint* paint);
/* what the driver lends the interval tables (ops_common.c): the pending intervals of chromsSorted[ci] as ib_add left them
 * (ib_begin forgets them), and the report's "%.*f" (NULL: not a case for the hand-rolled form, print through printf) */
int   ib_chromosomes      (void);
u32   ib_pending_of       (int ci, spec** s, u32** start, u32** end, valtype** val);
char* put_value_fixed     (char* p, valtype v, int precision);
/* what statsover, percentilesover, breadthover and correlateover share (ops_common.c): a table with one line per interval of a file, in file order --
 * chromosome, start and end as the file has them, then the operator's figures.  The file is read like mask's (read_interval
 * without a value column, place_interval), the intervals may overlap and come in any order; they are buffered with ib_add
 * and every ib_batch_limit() of them, and at the end of the file, each device answers those on its chromosomes in one call
 * and their lines are written.  The operator says how: */
typedef struct interval_table
	{
	size_t recSize;                               /* bytes of what is kept of an interval until its line is written */
	/* one device's share, that device selected: record i of `out` for interval i, [start[i], end[i]) of items[vec[i]]
	 * (d_in a chromosome's vector, d_out NULL: an operator with a second track names it there, as correlateover does) */
	void (*answer) (void* ctx, gdsp_batch_item* items, int m, u32* vec, u32* start, u32* end, u32 k, void* out);
	/* a line behind its end column, from its record, newline included, at p; -> behind what was written */
	char* (*put) (void* ctx, char* p, const void* rec, spec* s);
	size_t lineMax;                               /* the most characters of a line, beyond its chromosome's name */
	void (*header) (void* ctx, FILE* out);        /* writes the header lines; NULL: none */
	void*  ctx;
	u64    bases;                                 /* the run adds: the summed length of the intervals, */
	double msAll, msDevice, msFormat;             /* the time of the run, of its device calls and of formatting and writing */
	} interval_table;
void  interval_table_run  (char* name, char* filename, char* outFilename, int originOne, interval_table* t);
/* the head of those operators' control records, and what goes with it: the defaults; the options all of them take
 * (--output=, --min= --max= --precision=, --origin=, --debug, the file's name, the complaint about anything else), asked
 * after the operator has looked for its own; the complaints of the finished command line; the release of its strings;
 * interval_table_run with the head's file names, the intervals' bases added to the head; and the work trait (the signal
 * is only read, 8 B per base of the intervals' summed length since the last call) */
typedef struct interval_op
	{
	dspop       common;
	char*       filename;
	char*       outFilename;
	sample_opts sample;                           /* (its limits and precision; no window) */
	int         originOne;
	u64         bases;                            /* summed length of the intervals (--report=gpu) */
	} interval_op;
void  interval_op_init    (interval_op* h);
void  interval_op_take    (interval_op* h, char* name, char* arg);
void  interval_op_check   (interval_op* h, char* name);
void  interval_op_free    (interval_op* h);
void  interval_op_run     (interval_op* h, interval_table* t);
void  interval_op_work    (dspop* op, u64* bases, double* bytesPerBase);
/* the record percentilesover and breadthover keep of an interval: the size of its sample, a u32, and behind it n figures
 * of elemSize bytes (4 or 8) each, the first elemSize bytes into the record.  new: room for k intervals' counts and
 * figures as the library gives them; into: the k records at `out`, and the room is released */
typedef struct counted_figures { u32* count;  void* figures;  size_t k, n, elemSize; } counted_figures;
#define counted_figures_size(n, elemSize) (((size_t) (n) + 1) * (elemSize))
counted_figures counted_figures_new  (char* name, size_t k, size_t n, size_t elemSize);
void            counted_figures_into (counted_figures* f, void* out);
/* ops_correlate.c (correlate), shared with ops_lagcorr.c: the intervals of a file, read
 * by the rules of `add <file>`, into every chromosome's partner -- what `add <file>` would leave on an all-zero genome */
void  load_track_into_partners (char* name, char* filename, int valColumn, int originOne);

/* argument helpers used by every operator's parse function */
#define OP_SHORT(fn, text)                                                            \
void fn##_short (char* name, int nameWidth, FILE* f, char* indent)                    \
	{                                                                                 \
	int fillW = nameWidth-2 - (int) strlen (name);                                    \
	if (indent == NULL) indent = "";                                                  \
	if (fillW > 0) fprintf (f, "%s%s:%*s", indent, name, fillW+1, " ");               \
	else           fprintf (f, "%s%s: ", indent, name);                               \
	fprintf (f, text "\n");                                                           \
	}

#define is_opt3(arg, long_, short_)                                                   \
	((strcmp_prefix (arg, "--" long_ "=") == 0) || (strcmp_prefix (arg, short_ "=") == 0) \
	 || (strcmp_prefix (arg, "--" short_ "=") == 0))

#endif
