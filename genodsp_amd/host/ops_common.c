/* ops_common.c -- helpers shared by the operator files. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <ctype.h>
#include <float.h>
#include <math.h>
#include "genodsp_interface.h"
#include "utilities.h"
#include "host_services.h"

void* new_op (char* name, size_t bytes, int atRandom)
	{
	dspop* op = (dspop*) calloc (1, bytes);
	if (op == NULL) { fprintf (stderr, "[%s] failed to allocate control record (%d bytes)\n", name, (int) bytes);  exit (EXIT_FAILURE); }
	op->atRandom = atRandom;
	return op;
	}

void* must_alloc (void* p, const char* name)
	{
	if (p == NULL) { fprintf (stderr, "[%s] out of memory\n", name);  exit (EXIT_FAILURE); }
	return p;
	}

/* --origin=one|1|zero|0 of an operator with a coordinate convention of its own; true: `arg` was it */
int origin_opt_take (char* arg, int* originOne)
	{
	if ((strcmp (arg, "--origin=one") == 0)  || (strcmp (arg, "--origin=1") == 0)) { *originOne = true;   return true; }
	if ((strcmp (arg, "--origin=zero") == 0) || (strcmp (arg, "--origin=0") == 0)) { *originOne = false;  return true; }
	return false;
	}

/* --value=<col>, or --novalue / --novalues / --value=none, of an operator that reads a file of intervals; true: `arg`
 * was it, and *valColumn is the column counted from 0 (-1: the intervals carry no value) */
int value_column_take (char* name, char* arg, int* valColumn)
	{
	if ((strcmp (arg, "--novalue") == 0) || (strcmp (arg, "--novalues") == 0) || (strcmp (arg, "--value=none") == 0))
		{ *valColumn = -1;  return true; }
	if (strcmp_prefix (arg, "--value=") != 0) return false;
	int col = string_to_int (strchr (arg, '=') + 1) - 1;
	if (col == -1) chastise ("[%s] value column can't be 0 (\"%s\")\n", name, arg);
	if (col < 0)   chastise ("[%s] value column can't be negative (\"%s\")\n", name, arg);
	if (col < 3)   chastise ("[%s] value column can't be 1, 2 or 3 (\"%s\")\n", name, arg);
	*valColumn = col;
	return true;
	}

/* --sharding=bases, the reach of an operator (optraits): none for a per-base operator; for a window centred as bestmax
 * centres its own (minmax.c:1636-1640: [i-wLft, i+wRgt]), (W-1)/2 bases to the left and the rest to the right */
int reach_none (dspop* op, u32* left, u32* right) { *left = *right = 0;  return true; }

int reach_centred (u32 W, u32* left, u32* right) { *left = (W - 1) / 2;  *right = W - 1 - *left;  return true; }

/* --window=<n> and friends: zero and negatives are errors, 1-2 are raised to 3 with a
 * warning (sum.c:121-132, minmax.c:1116-1126) */
u32 window_arg (char* name, char* arg, char* argVal, const char* what)
	{
	int w = string_to_unitized_int (argVal, /*thousands*/ true);
	if (w == 0) chastise ("[%s] %s can't be zero (\"%s\")\n", name, what, arg);
	if (w < 0)  chastise ("[%s] %s can't be negative (\"%s\")\n", name, what, arg);
	if (w < 3) { fprintf (stderr, "[%s] WARNING: raising %s from %d to %d\n", name, what, w, 3);  w = 3; }
	return (u32) w;
	}

/* morphology.c:137-140, mask.c: a value that does not parse as a number is the name of
 * a variable some earlier operator (percentile) will have set by the time we run */
void value_or_variable (char* argVal, valtype* val, char** varName)
	{
	if (!try_string_to_valtype (argVal, val)) *varName = copy_string (argVal);
	}

/* <value|variable> for a level (localstats, localmad): a number, or something that can be the name of a variable (a
 * letter or underscore, then letters, digits, underscores and dots) */
void level_arg (char* name, char* arg, char* argVal, valtype* val, char** varName)
	{
	if (*varName != NULL) { free (*varName);  *varName = NULL; }
	value_or_variable (argVal, val, varName);
	if (*varName == NULL)
		{
		if (*val != *val) chastise ("[%s] \"%s\" is not a number\n", name, arg);
		return;
		}
	int ok = (isalpha ((unsigned char) argVal[0]) || (argVal[0] == '_'));
	for (char* c=argVal ; ok && (*c != 0) ; c++) ok = (isalnum ((unsigned char) *c) || (*c == '_') || (*c == '.'));
	if (!ok) chastise ("[%s] \"%s\" is neither a number nor the name of a variable\n", name, arg);
	}

/* logical.c:234-243: fetch the variable at first apply, say so, then forget the name */
void resolve_variable (dspop* op, char** varName, valtype* val, const char* role)
	{
	if (*varName == NULL) return;
	if (!named_global_exists (*varName, val))
		{
		fprintf (stderr, "[%s] attempt to use %s as %s failed (no such variable)\n", op->name, *varName, role);
		exit (EXIT_FAILURE);
		}
	fprintf (stderr, "[%s] using %s = " valtypeFmt " as %s\n", op->name, *varName, *val, role);
	free (*varName);
	*varName = NULL;
	}

/* ---- what the operators that only read the signal (percentile, stats, normalize, histogram, statsover) share ---- */

/* percentile.c:150-156: the sample is every base with any value, looked at one per window of the global --window= */
void sample_opts_init (sample_opts* o)
	{
	o->minAllowed = -valtypeMax;
	o->maxAllowed =  valtypeMax;
	o->window     = (u32) get_named_global ("windowSize", 1);
	if (o->window == 0) o->window = 1;
	o->precision  = -1;                                              /* -1: %.17g, every digit a double has */
	o->quiet      = false;
	}

/* --min= and --max=, and of --window= (W=), --precision= and --quiet (--silent) those the operator accepts
 * (SAMPLE_OPT_*); true when arg was one of them */
int sample_opts_take (sample_opts* o, char* name, char* arg, int accepts)
	{
	char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
	if ((accepts & SAMPLE_OPT_WINDOW) && is_opt3 (arg, "window", "W"))
		{
		int w = string_to_unitized_int (argVal, /*thousands*/ true);
		if (w == 0) w = 1;
		if (w < 0) chastise ("[%s] window size can't be negative (\"%s\")\n", name, arg);
		o->window = (u32) w;
		return true;
		}
	if (strcmp_prefix (arg, "--min=") == 0) { o->minAllowed = string_to_valtype (argVal);  return true; }
	if (strcmp_prefix (arg, "--max=") == 0) { o->maxAllowed = string_to_valtype (argVal);  return true; }
	if ((accepts & SAMPLE_OPT_PRECISION) && (strcmp_prefix (arg, "--precision=") == 0))
		{
		o->precision = string_to_int (argVal);
		if (o->precision < 0) chastise ("[%s] precision can't be negative (\"%s\")\n", name, arg);
		return true;
		}
	if ((accepts & SAMPLE_OPT_QUIET) && ((strcmp (arg, "--quiet") == 0) || (strcmp (arg, "--silent") == 0)))
		{ o->quiet = true;  return true; }
	return false;
	}

/* the signal's parts as the source table of gdsp_genome_stats / gdsp_genome_histogram (the caller frees it): every
 * device has finished what it was doing, each part's stream is its device's, and the device of part 0 is current */
int signal_sources (char* name, gdsp_xsum_source** sources)
	{
	sigpart* parts;
	int nsrc = signal_parts (&parts);
	gdsp_xsum_source* src = (gdsp_xsum_source*) calloc (nsrc? nsrc : 1, sizeof(gdsp_xsum_source));
	if (src == NULL) { fprintf (stderr, "[%s] out of memory\n", name);  exit (EXIT_FAILURE); }
	sync_all_devices ();
	for (int i=0 ; i<nsrc ; i++)
		{
		select_device_of (parts[i].s);
		src[i].d_v = parts[i].v;  src[i].n = parts[i].n;  src[i].first = parts[i].first;
		src[i].device = physical_device_of (parts[i].s);  src[i].stream = op_stream ();
		}
	if (nsrc > 0) select_device_of (parts[0].s);
	*sources = src;
	return nsrc;
	}

/* where an interval of a file-driven operator (add, ..., correlate) lies in chromosome s's vector: [start, end) of the
 * chromosome, the origin already taken off, as [*adjStart, *adjEnd) of the vector (add.c:245-270).  An interval beyond
 * the end of a chromosome that begins at 0 ends the run with the complaint; false: no base of it is in the vector */
int place_interval (char* name, char* filename, char* chrom, spec* s, u32 start, u32 end, u32* adjStart, u32* adjEnd)
	{
	*adjStart = start;  *adjEnd = end;
	if (s->start == 0)
		{
		if (end > s->length)
			{
			fprintf (stderr, "[%s] in \"%s\", %s %d %d is beyond the end of the chromosome (L=%d)\n",
			                 name, filename, chrom, start, end, s->length);
			exit (EXIT_FAILURE);
			}
		return true;
		}
	if (end <= s->start) return false;
	*adjEnd   = end - s->start;
	*adjStart = (start <= s->start)? 0 : start - s->start;
	if (*adjStart >= s->length) return false;
	if (*adjEnd   >= s->length) *adjEnd = s->length;
	return true;
	}

/* "%.17g", or valtypeFmtPrec with a precision (>= 0), into text[size]; -> what snprintf returns */
int format_value (char* text, size_t size, valtype v, int precision)
	{
	if (precision < 0) return snprintf (text, size, "%.17g", v);
	return snprintf (text, size, valtypeFmtPrec, precision, v);
	}

/* --output=<file>: where an operator's table goes -- the file, or stdout when there is none */
FILE* open_table (char* name, char* filename)
	{
	if (filename == NULL) return stdout;
	FILE* out = fopen (filename, "wt");
	if (out == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for writing\n", name, filename);  exit (EXIT_FAILURE); }
	return out;
	}

void close_table (FILE* out) { if (out != stdout) fclose (out);  else fflush (stdout); }

/* ---- the hand-rolled number formatting of the tables (statsover, segments) ---- */

char* put_unsigned (char* p, unsigned long long u)
	{
	char digits[24];
	int  n = 0;
	do { digits[n++] = (char) ('0' + u % 10);  u /= 10; } while (u != 0);
	while (n > 0) *(p++) = digits[--n];
	return p;
	}

static int clipped (int written) { return (written > 399)? 399 : written; }     /* (what snprintf kept of a longer text) */

/* format_value's text, at most 400 characters of it.  Integers below 10^15 (read depth, and its sums)
 * and fixed-point values take the hand-rolled forms: the same characters as printf's */
char* put_value (char* p, valtype v, int precision)
	{
	if (precision >= 0)
		{
		char* q = put_value_fixed (p, v, precision);
		if (q != NULL) return q;
		return p + clipped (format_value (p, 400, v, precision));
		}
	if ((fabs (v) < 1e15) && (v == floor (v)) && ((v != 0) || !signbit (v)))
		{
		if (v < 0) *(p++) = '-';
		return put_unsigned (p, (unsigned long long) fabs (v));
		}
	return p + clipped (format_value (p, 400, v, precision));
	}

/* the figures of an interval or segment behind the three leading columns of its line: tab, count, tab, sum, then mean,
 * min, max and the summit (chromStart + maxpos, + 1 when originOne), or four NA when nothing was sampled; the line ends
 * here.  At most 6 tabs and a newline, two integers of at most 20 digits and four values of at most 400 characters:
 * 1647 characters, inside the 2200 / 2400 the callers reserve per line beyond the chromosome's name */
char* put_interval_figures (char* p, const gdsp_interval_stat* stat, u32 chromStart, int originOne, int precision)
	{
	*(p++) = '\t';  p = put_unsigned (p, stat->count);
	*(p++) = '\t';  p = put_value (p, stat->sum, precision);
	if (stat->count == 0) { memcpy (p, "\tNA\tNA\tNA\tNA\n", 13);  return p + 13; }
	*(p++) = '\t';  p = put_value (p, stat->mean, precision);
	*(p++) = '\t';  p = put_value (p, stat->min,  precision);
	*(p++) = '\t';  p = put_value (p, stat->max,  precision);
	*(p++) = '\t';  p = put_unsigned (p, (unsigned long long) chromStart + stat->maxpos + (originOne? 1 : 0));
	*(p++) = '\n';
	return p;
	}

/* ------------------------------------------------------------- anchors of a file (profileover, matrixover) ---- */
static long long bases_arg (char* name, char* arg, char* argVal, const char* what)
	{
	int n = string_to_unitized_int (argVal, /*thousands*/ true);
	if (n < 0) chastise ("[%s] %s can't be negative (\"%s\")\n", name, what, arg);
	return n;
	}

void anchor_opts_init (anchor_opts* o)
	{
	memset (o, 0, sizeof(*o));
	o->originOne    = (int) get_named_global ("originOne", false);
	o->strandColumn = -1;
	o->anchor       = anchor_start;
	o->bin          = 1;
	}

int anchor_opts_take (anchor_opts* o, char* name, char* arg)
	{
	char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
	if (strcmp_prefix (arg, "--flank=") == 0)      { o->flank      = bases_arg (name, arg, argVal, "the flank");            o->haveFlank = true;  return true; }
	if (strcmp_prefix (arg, "--upstream=") == 0)   { o->upstream   = bases_arg (name, arg, argVal, "the upstream reach");   o->haveUp    = true;  return true; }
	if (strcmp_prefix (arg, "--downstream=") == 0) { o->downstream = bases_arg (name, arg, argVal, "the downstream reach"); o->haveDown  = true;  return true; }
	if (strcmp_prefix (arg, "--bin=") == 0)
		{
		int b = string_to_unitized_int (argVal, /*thousands*/ true);
		if (b < 1) chastise ("[%s] the bin must be at least one base (\"%s\")\n", name, arg);
		o->bin = b;
		return true;
		}
	if (strcmp_prefix (arg, "--anchor=") == 0)
		{
		if      (strcmp (argVal, "start")  == 0) o->anchor = anchor_start;
		else if (strcmp (argVal, "end")    == 0) o->anchor = anchor_end;
		else if ((strcmp (argVal, "center") == 0) || (strcmp (argVal, "centre") == 0)) o->anchor = anchor_center;
		else chastise ("[%s] the anchor is the interval's start, end or center (\"%s\")\n", name, arg);
		return true;
		}
	if (strcmp_prefix (arg, "--strand=") == 0)
		{
		int col = string_to_int (argVal) - 1;
		if (col == -1) chastise ("[%s] strand column can't be 0 (\"%s\")\n", name, arg);
		if (col < 0)   chastise ("[%s] strand column can't be negative (\"%s\")\n", name, arg);
		if (col < 3)   chastise ("[%s] strand column can't be 1, 2 or 3 (\"%s\")\n", name, arg);
		o->strandColumn = col;
		return true;
		}
	if (is_opt3 (arg, "window", "W"))
		chastise ("[%s] every base the anchors reach is looked at: no window (\"%s\")\n", name, arg);
	return origin_opt_take (arg, &o->originOne);
	}

void anchor_opts_check (anchor_opts* o, char* name)
	{
	if (o->haveFlank && (o->haveUp || o->haveDown))
		chastise ("[%s] Can't use --flank with --upstream or --downstream\n", name);
	if (!o->haveFlank && !(o->haveUp && o->haveDown))
		chastise ("[%s] no offsets were provided (--flank=<bases>, or --upstream=<bases> and --downstream=<bases>)\n", name);
	if (o->haveFlank) o->upstream = o->downstream = o->flank;
	const long long noffsets = o->upstream + o->downstream + 1;
	if (noffsets > GDSP_PROFILE_MAX_OFFSETS)
		chastise ("[%s] at most %d offsets can be computed at once (%lld..%lld)\n", name, GDSP_PROFILE_MAX_OFFSETS, -o->upstream, o->downstream);
	if (noffsets % o->bin != 0)
		chastise ("[%s] the bin must divide the number of offsets (%lld does not divide %lld)\n", name, o->bin, noffsets);
	}

/* a line of the file as read_interval's serial loop (ingest.c) takes it -- track lines, blank lines and comments are
 * passed over; chromosome, start and end are the first three fields -- and with it the strand: minus when field
 * strandCol (zero-based; -1: none) begins with '-'.  false at the end of the file */
int read_anchor_line (char* name, char* filename, FILE* f, char* line, int lineLen, u64* lineNumber, int strandCol,
                      char** _chrom, u32* _start, u32* _end, int* _minus)
	{
	char *scan, *mark, *field;
	for (;;)
		{
		if (fgets (line, lineLen, f) == NULL) return false;
		(*lineNumber)++;
		size_t len = strlen (line);
		if ((len != 0) && (line[len-1] != '\n') && !feof (f))
			{ fprintf (stderr, "[%s] in \"%s\", line %llu is longer than internal buffer\n", name, filename, (unsigned long long) *lineNumber);  exit (EXIT_FAILURE); }
		if (strcmp_prefix (line, "track ") == 0) continue;
		scan = skip_whitespace (line);
		if ((*scan == 0) || (*scan == '#')) continue;
		break;
		}
	const char* missing = NULL;
	char* chrom = scan = line;
	if (*scan == ' ') missing = "chromosome";
	mark = skip_darkspace (scan);  scan = skip_whitespace (mark);  if (*mark != 0) *mark = 0;
	if ((missing == NULL) && (*scan == 0)) missing = "interval start";
	field = scan;
	mark = skip_darkspace (scan);  scan = skip_whitespace (mark);  if (*mark != 0) *mark = 0;
	u32 start = (missing == NULL)? (u32) string_to_u32 (field) : 0;
	if ((missing == NULL) && (*scan == 0)) missing = "interval end";
	field = scan;
	mark = skip_darkspace (scan);  scan = skip_whitespace (mark);  if (*mark != 0) *mark = 0;
	u32 end = (missing == NULL)? (u32) string_to_u32 (field) : 0;
	int minus = false;
	for (int col=3 ; (missing == NULL) && (col<=strandCol) ; col++)
		{
		if (*scan == 0) { missing = "strand";  break; }
		field = scan;
		mark = skip_darkspace (scan);  scan = skip_whitespace (mark);
		if (col == strandCol) minus = (field[0] == '-');
		}
	if (missing != NULL)
		{
		fprintf (stderr, "[%s] in \"%s\", line %llu contains no %s\n", name, filename, (unsigned long long) *lineNumber, missing);
		exit (EXIT_FAILURE);
		}
	*_chrom = chrom;  *_start = start;  *_end = end;  *_minus = minus;
	return true;
	}

/* where the anchor of the zero-based half-open interval [s, e), s < e, lies */
long long anchor_of (long long s, long long e, int minus, int anchor)
	{
	const long long half = (e - s - 1) / 2;
	switch (anchor)
		{
		case anchor_end:    return minus? s : e - 1;
		case anchor_center: return minus? e - 1 - half : s + half;
		default:            return minus? e - 1 : s;
		}
	}

/* the file: every interval's anchor, to its chromosome (parts[i] of the whole-chromosome signal; anc[i] zeroed by the
 * caller).  `used`, when not NULL, sees every anchor that is used, in the file's order */
void read_anchor_file (char* name, char* filename, const anchor_opts* o, const sigpart* parts, int nsrc, anchors* anc,
                       u64* _numRead, u64* _numUsed, u64* _numSkipped, anchor_used_fn used, void* usedCtx)
	{
	const long long org = o->originOne? 1 : 0;
	FILE* f = fopen (filename, "rt");
	if (f == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for reading\n", name, filename);  exit (EXIT_FAILURE); }
	for (int i=0 ; chromsSorted[i]!=NULL ; i++) chromsSorted[i]->flag = false;
	char  line[1001], prevChrom[1001];
	char* chrom;
	u32   start, end;
	int   minus, at = -1;
	u64   lineNumber = 0, numRead = 0, numUsed = 0, numSkipped = 0;
	spec* s = NULL;
	prevChrom[0] = 0;
	while (read_anchor_line (name, filename, f, line, sizeof(line), &lineNumber, o->strandColumn, &chrom, &start, &end, &minus))
		{
		if (strcmp (chrom, prevChrom) != 0)
			{
			s = find_chromosome_spec (chrom);  safe_strncpy (prevChrom, chrom, sizeof(prevChrom)-1);
			at = -1;
			for (int i=0 ; (s!=NULL) && (i<nsrc) ; i++) { if (parts[i].s == s) { at = i;  break; } }
			if (at < 0) s = NULL;
			}
		if (s == NULL) continue;
		if (!s->flag) { if (trackOperations) fprintf (stderr, "%s(%s)\n", name, chrom);  s->flag = true; }
		numRead++;
		const long long is = (long long) start - org, ie = (long long) end;
		long long p = -1;
		if (is < ie) p = anchor_of (is, ie, minus, o->anchor) - (long long) s->start;
		if ((is >= ie) || (p < 0) || (p >= (long long) parts[at].n)) { numSkipped++;  continue; }
		anchors* a = &anc[at];
		if (a->count == a->cap)
			{
			if (a->cap >= (1u << 31)) { fprintf (stderr, "[%s] too many anchors on %s\n", name, chrom);  exit (EXIT_FAILURE); }
			a->cap   = (a->cap == 0)? 1024 : 2*a->cap;
			a->pos   = (u32*) must_alloc (realloc (a->pos,   a->cap * sizeof(u32)), name);
			a->minus = (u32*) must_alloc (realloc (a->minus, a->cap * sizeof(u32)), name);
			}
		if (used != NULL) used (usedCtx, at, a->count, start, end, minus);
		a->pos[a->count] = (u32) p;  a->minus[a->count] = (u32) minus;  a->count++;
		numUsed++;
		}
	fclose (f);
	*_numRead = numRead;  *_numUsed = numUsed;  *_numSkipped = numSkipped;
	}

/* ---------------------------------------------- a table with one line per used row (matrixover, regionsover) ---- */
const char* const figureNames[5] = { "mean", "sum", "count", "min", "max" };       /* GDSP_MATRIX_* */

int figure_opt_take (char* name, char* arg, int* what)
	{
	if (strcmp_prefix (arg, "--as=") != 0) return false;
	*what = -1;
	for (int k=0 ; k<5 ; k++) { if (strcmp (strchr (arg, '=') + 1, figureNames[k]) == 0) *what = k; }
	if (*what < 0) chastise ("[%s] the figure is mean, sum, count, min or max (\"%s\")\n", name, arg);
	return true;
	}

void rowlist_add (rowlist* l, int part, u32 index, u32 start, u32 end, u32 length, int minus)
	{
	if (l->count == l->cap)
		{
		l->cap  = (l->cap == 0)? 1024 : 2*l->cap;
		l->rows = (rowrec*) must_alloc (realloc (l->rows, l->cap * sizeof(rowrec)), l->name);
		}
	rowrec* r = &l->rows[l->count++];
	r->part = (u32) part;  r->index = index;  r->start = start;  r->end = end;  r->length = length;  r->minus = minus;
	}

/* the whole table lives on the host: refused before any device work when it is too large */
u64 row_table_cells (char* name, u64 numUsed, u32 ncols, const char* complaint)
	{
	const u64 cells = numUsed * ncols;
	if (cells > ROW_TABLE_MAX_CELLS)
		{
		fprintf (stderr, complaint, name, (unsigned long long) numUsed, ncols, (unsigned long long) cells, (unsigned long long) ROW_TABLE_MAX_CELLS);
		exit (EXIT_FAILURE);
		}
	return cells;
	}

double* row_table_part (char* name, const sigpart* part, u32 count, u32 ncols, const valtype** d_v, u32* n, int* device, void** stream)
	{
	select_device_of (part->s);
	*d_v = part->v;  *n = part->n;
	*device = physical_device_of (part->s);  *stream = op_stream ();
	return (count == 0)? NULL : (double*) must_alloc (malloc ((size_t) count * ncols * sizeof(double)), name);
	}

void row_table_print (char* name, FILE* out, const rowlist* list, double* const* table, u32 ncols, const sigpart* parts,
                      int strandColumn, int withLength, int precision)
	{
	enum { textLen = 1 << 16 };
	char* text = (char*) must_alloc (malloc (textLen), name);
	for (u64 r=0 ; r<list->count ; r++)
		{
		const rowrec* rr = &list->rows[r];
		const double* x  = table[rr->part] + (size_t) rr->index * ncols;
		const char strand = (strandColumn < 0)? '.' : (rr->minus? '-' : '+');
		fprintf (out, "%s\t%u\t%u\t%c", parts[rr->part].s->chrom, rr->start, rr->end, strand);
		if (withLength) fprintf (out, "\t%u", rr->length);
		char* p = text;
		for (u32 j=0 ; j<ncols ; j++)
			{
			*(p++) = '\t';
			if (isnan (x[j])) { memcpy (p, "NA", 2);  p += 2; }
			else              p = put_value (p, x[j], precision);
			if (p - text > textLen - 450) { fwrite (text, 1, (size_t) (p - text), out);  p = text; }
			}
		*(p++) = '\n';
		fwrite (text, 1, (size_t) (p - text), out);
		}
	free (text);
	}

void row_table_report (char* rowsName, u64 numUsed, u64 cells, int quiet)
	{
	set_named_global (rowsName, (valtype) numUsed);
	set_named_global ("cells",  (valtype) cells);
	if (!quiet) fprintf (stderr, "%s is %llu, cells is %llu\n", rowsName, (unsigned long long) numUsed, (unsigned long long) cells);
	}

/* -------- a table with one line per interval of a file (statsover, percentilesover, breadthover, correlateover) ---- */
/* a kept interval as its line names it; its record arrives in rec under the same serial number */
typedef struct itrow { spec* s;  u32 fileStart, fileEnd; } itrow;

typedef struct itbatch
	{
	itrow* rows;   char* rec;   size_t cap;                     /* by serial number */
	u32   *vec, *start, *end, *serial;  char* out;  size_t ivCap;      /* one device's share, as the library takes it */
	char*  text;   size_t textCap;
	} itbatch;

/* the pending intervals' records, device by device (one call each), then their lines in file order */
static void interval_table_flush (char* name, interval_table* t, itbatch* b, u64 pending, FILE* f)
	{
	const int numChroms = ib_chromosomes ();
	if (pending == 0) return;
	gdsp_batch_item* items = (gdsp_batch_item*) must_alloc (calloc (numChroms + 1, sizeof(gdsp_batch_item)), name);
	sync_all_devices ();
	const double t0 = now_ms ();
	for (int d=0 ; d<device_count_in_use () ; d++)
		{
		int    m = 0;
		size_t k = 0, want = 0;
		spec*  first = NULL;
		for (int ci=0 ; ci<numChroms ; ci++)
			{
			spec* s;  u32 *start, *end;  valtype* val;
			u32 count = ib_pending_of (ci, &s, &start, &end, &val);
			if ((count != 0) && (device_index_of (s) == d)) want += count;
			}
		if (want == 0) continue;
		if (want > b->ivCap)
			{
			free (b->vec);  free (b->start);  free (b->end);  free (b->serial);  free (b->out);
			b->vec    = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->start  = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->end    = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->serial = (u32*) must_alloc (malloc (want * sizeof(u32)), name);
			b->out    = (char*) must_alloc (malloc (want * t->recSize), name);
			b->ivCap  = want;
			}
		for (int ci=0 ; ci<numChroms ; ci++)
			{
			spec* s;  u32 *start, *end;  valtype* val;
			u32 count = ib_pending_of (ci, &s, &start, &end, &val);
			if ((count == 0) || (device_index_of (s) != d)) continue;
			if (first == NULL) first = s;
			items[m].d_in = s->valVector;  items[m].d_out = NULL;  items[m].n = s->length;
			for (u32 i=0 ; i<count ; i++, k++)
				{ b->vec[k] = (u32) m;  b->start[k] = start[i];  b->end[k] = end[i];  b->serial[k] = (u32) val[i]; }
			m++;
			}
		select_device_of (first);
		t->answer (t->ctx, items, m, b->vec, b->start, b->end, (u32) k, b->out);
		for (size_t i=0 ; i<k ; i++) memcpy (b->rec + b->serial[i] * t->recSize, b->out + i * t->recSize, t->recSize);
		}
	free (items);
	select_device_of (chromsSorted[0]);
	const double t1 = now_ms ();

	size_t len = 0;
	for (u64 r=0 ; r<pending ; r++)
		{
		const itrow* w = &b->rows[r];
		const size_t chromLen = strlen (w->s->chrom);
		if (len + chromLen + t->lineMax > b->textCap)
			{
			if (len != 0) { fwrite (b->text, 1, len, f);  len = 0; }
			if (chromLen + t->lineMax > b->textCap)
				{
				b->textCap = (1u << 20) + chromLen + t->lineMax;
				b->text = (char*) must_alloc (realloc (b->text, b->textCap), name);
				}
			}
		char* p = b->text + len;
		memcpy (p, w->s->chrom, chromLen);  p += chromLen;  *(p++) = '\t';
		p = put_unsigned (p, w->fileStart);  *(p++) = '\t';
		p = put_unsigned (p, w->fileEnd);
		p = t->put (t->ctx, p, b->rec + r * t->recSize, w->s);
		len = (size_t) (p - b->text);
		}
	if (len != 0) fwrite (b->text, 1, len, f);
	t->msDevice += t1 - t0;  t->msFormat += now_ms () - t1;
	ib_begin ();                                               /* forget them */
	}

void interval_table_run (char* name, char* filename, char* outFilename, int originOne, interval_table* t)
	{
	char    line[1001], prevChrom[1001];
	char*   chrom;
	spec*   s = NULL;
	u32     start, end, o = originOne? 1 : 0;
	valtype val;
	itbatch b;
	memset (&b, 0, sizeof(b));

	const double tStart = now_ms ();
	FILE* f = fopen (filename, "rt");
	if (f == NULL) { fprintf (stderr, "[%s] can't open \"%s\" for reading\n", name, filename);  exit (EXIT_FAILURE); }
	FILE* out = open_table (name, outFilename);
	for (int i=0 ; chromsSorted[i]!=NULL ; i++) chromsSorted[i]->flag = false;
	if (t->header != NULL) t->header (t->ctx, out);

	ib_begin ();
	prevChrom[0] = 0;
	while (read_interval (f, line, sizeof(line), /*valCol*/ -1, &chrom, &start, &end, &val))
		{
		if (strcmp (chrom, prevChrom) != 0)
			{ s = find_chromosome_spec (chrom);  safe_strncpy (prevChrom, chrom, sizeof(prevChrom)-1); }
		if (s == NULL) continue;
		if (!s->flag) { if (trackOperations) fprintf (stderr, "%s(%s)\n", name, chrom);  s->flag = true; }

		const u32 fileStart = start;
		start -= o;
		u32 adjStart, adjEnd;
		if (!place_interval (name, filename, chrom, s, start, end, &adjStart, &adjEnd)) continue;
		if (adjStart >= adjEnd) continue;                      /* (an empty interval has no sample and no line) */
		const u64 serial = ib_pending ();
		if (serial >= b.cap)
			{
			b.cap  = (b.cap == 0)? 4096 : 2*b.cap;
			b.rows = (itrow*) must_alloc (realloc (b.rows, b.cap * sizeof(itrow)), name);
			b.rec  = (char*) must_alloc (realloc (b.rec, b.cap * t->recSize), name);
			}
		b.rows[serial].s = s;  b.rows[serial].fileStart = fileStart;  b.rows[serial].fileEnd = end;
		ib_add (s, adjStart, adjEnd, (valtype) serial);
		t->bases += adjEnd - adjStart;
		if (ib_pending () >= ib_batch_limit ()) interval_table_flush (name, t, &b, ib_pending (), out);
		}
	fclose (f);
	interval_table_flush (name, t, &b, ib_pending (), out);
	close_table (out);
	t->msAll += now_ms () - tStart;
	free (b.rows);  free (b.rec);  free (b.vec);  free (b.start);  free (b.end);  free (b.serial);  free (b.out);  free (b.text);
	}

/* the head the operators of such a table embed (host_services.h) */
void interval_op_init (interval_op* h)
	{
	sample_opts_init (&h->sample);
	h->originOne = (int) get_named_global ("originOne", false);
	}

void interval_op_take (interval_op* h, char* name, char* arg)
	{
	if (strcmp_prefix (arg, "--output=") == 0)
		{ if (h->outFilename != NULL) free (h->outFilename);  h->outFilename = copy_string (strchr (arg, '=') + 1);  return; }
	if (sample_opts_take (&h->sample, name, arg, SAMPLE_OPT_PRECISION)) return;
	if (origin_opt_take (arg, &h->originOne)) return;
	if (strcmp (arg, "--debug") == 0) return;
	if (strcmp_prefix (arg, "--") == 0) chastise ("[%s] Can't understand \"%s\"\n", name, arg);
	if (h->filename == NULL) { h->filename = copy_string (arg);  return; }
	chastise ("[%s] Can't understand \"%s\"\n", name, arg);
	}

void interval_op_check (interval_op* h, char* name)
	{
	if (h->filename == NULL) { fprintf (stderr, "[%s] no filename was provided\n", name);  exit (EXIT_FAILURE); }
	if (h->sample.minAllowed > h->sample.maxAllowed) chastise ("[%s] --min can't be above --max\n", name);
	}

void interval_op_free (interval_op* h)
	{
	if (h->filename    != NULL) free (h->filename);
	if (h->outFilename != NULL) free (h->outFilename);
	}

void interval_op_run (interval_op* h, interval_table* t)
	{
	interval_table_run (h->common.name, h->filename, h->outFilename, h->originOne, t);
	h->bases += t->bases;
	}

void interval_op_work (dspop* op, u64* bases, double* bytesPerBase)
	{ *bases = ((interval_op*) op)->bases;  ((interval_op*) op)->bases = 0;  *bytesPerBase = 8; }

counted_figures counted_figures_new (char* name, size_t k, size_t n, size_t elemSize)
	{
	counted_figures f = { (u32*) must_alloc (malloc (k * sizeof(u32)), name), must_alloc (malloc (k * n * elemSize), name), k, n, elemSize };
	return f;
	}

void counted_figures_into (counted_figures* f, void* out)
	{
	const size_t bytes = f->n * f->elemSize;
	for (size_t i=0 ; i<f->k ; i++)
		{
		char* r = (char*) out + i * counted_figures_size (f->n, f->elemSize);
		*(u32*) r = f->count[i];
		memcpy (r + f->elemSize, (char*) f->figures + i * bytes, bytes);
		}
	free (f->count);  free (f->figures);
	}
