/* ops_breadthover.c -- breadthover (device shim).  Not an operator of the reference: a table with one line per interval of
 * a file -- the size of the interval's sample and, for every threshold asked for, the number (or the share) of its bases
 * at or above that threshold: "what share of this target is covered at least 20x", the figure exome, panel and amplicon
 * QC is made of.  `= binarize T = statsover f` answers one threshold, with binarize's `>`, destroys the signal and takes
 * a pass per threshold; percentilesover answers the inverse question.  The signal is not modified and no variable is set.
 *
 * The file is read, the intervals are batched and the lines are written by the half shared with statsover and
 * percentilesover, which also takes the options the three have in common (interval_table_run, interval_op: ops_common.c;
 * host_services.h says how): the intervals may overlap and come in any order, and every ib_batch_limit() of them, and at
 * the end of the file, each device answers the intervals on its chromosomes in one call (gdsp_interval_breadth_batch,
 * include/genodsp_hip.h: every figure an integer, a function of the interval's sample alone).  What is this operator's
 * own is that call, the thresholds -- numbers, or variables fetched when the operator runs --, the header with a column
 * per threshold and the figures of a line.
 *
 * The driver finds this operator through opgroup_breadthover, at the end of this file (host_services.h); every call into
 * the device library for it stays here. */
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include "genodsp_interface.h"
#include "genodsp_hip.h"
#include "utilities.h"
#include "host_services.h"

dspprototypes(op_breadthover)

typedef struct dspop_breadthover
	{
	interval_op head;
	int         tiesAbove;                      /* a base equal to the threshold counts ("at least"): the default */
	int         asFraction;
	valtype     thresholds[GDSP_INTERVAL_THRESHOLDS_MAX];   /* in the order given */
	char*       varNames[GDSP_INTERVAL_THRESHOLDS_MAX];     /* those still to be fetched (resolve_variable) */
	char*       labels[GDSP_INTERVAL_THRESHOLDS_MAX];       /* as the user spelled them */
	int         numThresholds;
	} dspop_breadthover;

static void op_breadthover_usage_text (char* name, FILE* f, char* indent)
	{
	if (indent == NULL) indent = "";
	fprintf (f, "%sPrint one line per interval of a file, in file order: chromosome, start, end, then the\n", indent);
	fprintf (f, "%snumber of values looked at and, for every threshold asked for, how many of them are at least\n", indent);
	fprintf (f, "%sthat threshold (breadth of coverage at that depth). Intervals may overlap and come in any\n", indent);
	fprintf (f, "%sorder. An interval with nothing to look at prints zeros (NA as fractions). The signal is not\n", indent);
	fprintf (f, "%smodified. Not in genodsp.\n\n", indent);
	fprintf (f, "%susage: %s <filename> [options]\n", indent, name);
	fprintf (f, "%s  --thresholds=<t>[,<t>...]  numbers or variables, at most %d (default: 1, the covered bases)\n", indent, GDSP_INTERVAL_THRESHOLDS_MAX);
	fprintf (f, "%s  --ties:above|below       whether values equal to a threshold count (above, the default: \"at\n", indent);
	fprintf (f, "%s                           least\") or not; note that segments and binarize default to below\n", indent);
	fprintf (f, "%s  --as=count|fraction      print bases (default) or their share of the values looked at\n", indent);
	fprintf (f, "%s  --output=<file>          write the table there (default: stdout, when the operator runs)\n", indent);
	fprintf (f, "%s  --min=<value> --max=<value>  ignore values outside this range\n", indent);
	fprintf (f, "%s  --precision=<number>     digits after the point of a fraction (default: all of them)\n", indent);
	fprintf (f, "%s  --origin=one|zero        coordinate convention of the file\n", indent);
	}

static void forget_thresholds (dspop_breadthover* op)
	{
	for (int j=0 ; j<op->numThresholds ; j++)
		{
		if (op->varNames[j] != NULL) free (op->varNames[j]);
		if (op->labels[j]   != NULL) free (op->labels[j]);
		op->varNames[j] = op->labels[j] = NULL;
		}
	op->numThresholds = 0;
	}

static void take_thresholds (dspop_breadthover* op, char* name, char* arg, char* list)
	{
	char* text = copy_string (list);
	forget_thresholds (op);
	for (char* t=text ; t!=NULL ; )
		{
		char* comma = strchr (t, ',');
		if (comma != NULL) *(comma++) = 0;
		if (op->numThresholds == GDSP_INTERVAL_THRESHOLDS_MAX)
			chastise ("[%s] at most %d thresholds can be asked for (\"%s\")\n", name, GDSP_INTERVAL_THRESHOLDS_MAX, arg);
		const int j = op->numThresholds++;
		op->labels[j] = copy_string (t);
		level_arg (name, arg, t, &op->thresholds[j], &op->varNames[j]);      /* a number that is not NaN, or a variable's name */
		t = comma;
		}
	free (text);
	}

dspop* op_breadthover_parse (char* name, int argc, char** argv)
	{
	dspop_breadthover* op = (dspop_breadthover*) new_op (name, sizeof(dspop_breadthover), true);
	interval_op_init (&op->head);
	op->tiesAbove = true;
	take_thresholds (op, name, (char*) "--thresholds=1", (char*) "1");
	for ( ; argc > 0 ; argv++, argc--)
		{
		char* arg = argv[0];
		char* argVal = strchr (arg, '=');  if (argVal != NULL) argVal++;
		if ((strcmp_prefix (arg, "--thresholds=") == 0) || (strcmp_prefix (arg, "--threshold=") == 0))
			{ take_thresholds (op, name, arg, argVal);  continue; }
		if ((strcmp (arg, "--ties:above") == 0) || (strcmp (arg, "--ties=above") == 0)) { op->tiesAbove = true;   continue; }
		if ((strcmp (arg, "--ties:below") == 0) || (strcmp (arg, "--ties=below") == 0)) { op->tiesAbove = false;  continue; }
		if (strcmp_prefix (arg, "--as=") == 0)
			{
			if      (strcmp (argVal, "count")    == 0) op->asFraction = false;
			else if (strcmp (argVal, "fraction") == 0) op->asFraction = true;
			else chastise ("[%s] --as= takes count or fraction (\"%s\")\n", name, arg);
			continue;
			}
		interval_op_take (&op->head, name, arg);
		}
	interval_op_check (&op->head, name);
	return (dspop*) op;
	}

void op_breadthover_free (dspop* op)
	{
	forget_thresholds ((dspop_breadthover*) op);
	interval_op_free ((interval_op*) op);
	free (op);
	}

/* ------------------------------------------------------------------------------------- the table's figures ---- */
/* what is kept of an interval: the size of its sample and, in the order asked for, its numThresholds counts */
typedef struct breadthrec { u32 count;  u32 atleast[]; } breadthrec;
#define breadthrec_size(nt) counted_figures_size (nt, sizeof(u32))
_Static_assert (__builtin_offsetof (breadthrec, count) == 0 && __builtin_offsetof (breadthrec, atleast) == sizeof(u32), "counted_figures' record");

/* one device's share in one call */
static void answer_breadth (void* ctx, gdsp_batch_item* items, int m, u32* vec, u32* start, u32* end, u32 k, void* out)
	{
	dspop_breadthover* op = (dspop_breadthover*) ctx;
	char* name = op->head.common.name;
	counted_figures f = counted_figures_new (name, k, (size_t) op->numThresholds, sizeof(u32));
	check_gdsp (gdsp_interval_breadth_batch (items, m, vec, start, end, k, op->thresholds, op->numThresholds, !op->tiesAbove,
	                                         op->head.sample.minAllowed, op->head.sample.maxAllowed, f.count, (u32*) f.figures, op_stream ()), name);
	counted_figures_into (&f, out);
	}

/* a line: the name, two coordinates and the count (at most 20 digits each), nt figures of at most 400 characters, tabs */
#define breadth_line_max(nt) (100 + 401 * (size_t) (nt))

static char* put_breadth (void* ctx, char* p, const void* rec, arg_dont_complain(spec* s))
	{
	dspop_breadthover* op = (dspop_breadthover*) ctx;
	const breadthrec* r = (const breadthrec*) rec;
	*(p++) = '\t';
	p = put_unsigned (p, r->count);
	for (int j=0 ; j<op->numThresholds ; j++)
		{
		*(p++) = '\t';
		if      (!op->asFraction) p = put_unsigned (p, r->atleast[j]);
		else if (r->count == 0)   { *(p++) = 'N';  *(p++) = 'A'; }
		else                      p = put_value (p, (double) r->atleast[j] / (double) r->count, op->head.sample.precision);   /* one IEEE division */
		}
	*(p++) = '\n';
	return p;
	}

/* the header: a column per threshold, ge (or gt) and the threshold as the user spelled it */
static void put_header (void* ctx, FILE* out)
	{
	dspop_breadthover* op = (dspop_breadthover*) ctx;
	fputs ("#chrom\tstart\tend\tcount", out);
	for (int j=0 ; j<op->numThresholds ; j++) fprintf (out, "\t%s%s", op->tiesAbove? "ge" : "gt", op->labels[j]);
	fputc ('\n', out);
	}

void op_breadthover_apply (dspop* _op, arg_dont_complain(char* vName), arg_dont_complain(u32 vLen), arg_dont_complain(valtype* v))
	{
	dspop_breadthover* op = (dspop_breadthover*) _op;
	for (int j=0 ; j<op->numThresholds ; j++)
		{
		resolve_variable (_op, &op->varNames[j], &op->thresholds[j], "threshold");
		if (op->thresholds[j] != op->thresholds[j]) chastise ("[%s] threshold %s is not a number\n", _op->name, op->labels[j]);
		}
	interval_table t = { breadthrec_size (op->numThresholds), answer_breadth, put_breadth, breadth_line_max (op->numThresholds), put_header, op, 0, 0, 0, 0 };
	interval_op_run (&op->head, &t);
	}

OP_SHORT (op_breadthover, "print the bases at or above each threshold over each interval of a file (not in genodsp)")
void op_breadthover_usage (char* name, FILE* f, char* indent) { op_breadthover_usage_text (name, f, indent); }

static const dspinfo breadthoverRows[] =
	{ dspinforecord("breadthover", op_breadthover), dspinfoalias ("breadth_over"), dspinfoalias ("coverageover"),
	  dspinfoalias ("coverage_over"), dspinfoalias ("thresholdsover") };
static const optraits breadthoverTraits[] = { { op_breadthover_apply, true, false, NULL, NULL, interval_op_work } };
const opgroup opgroup_breadthover = OPGROUP (breadthoverRows, breadthoverTraits, NULL);
